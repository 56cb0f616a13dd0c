/*
 * cw_engine.cpp -- the engine of libconsent_amd.so, host side (C ABI: include/consent_amd.h; inspection: csrc/cw_private.h).  In this order: the launch
 * table (every kernel's dynamic LDS size, named once); one device run = validate, plan and bind (cw_plan.h -> DevScratch), launch shape (grids and routing
 * from batch and knobs), enqueue (the order of a step); engine life cycle (cw_create / cw_destroy: streams in a fixed order of creation); per-stage timing
 * and the inspection entry points; the launchers of the path's neighbours (pile extraction, result planning, read re-assembly); host batches (cw_submit /
 * cw_wait) and the loop that runs a batch again with a larger plan (cw_run, cw_run_device_sync); the POA stage alone on a batch of groups (cw_poa_run_device,
 * cw_poa_run: kernels in cw_poa_op.h, the same enqueue_poa_stage as a window run); the re-assembly's local aligner alone on a batch of groups
 * (cw_sw_run_device, cw_sw_run: kernels in cw_sw_op.h; cw_sw_path_run_device, cw_sw_path_run: cw_sw_path.h; cw_pileup_run_device, cw_pileup_run: cw_pileup.h; cw_sw_cut_run_device, cw_sw_cut_run,
 * cw_cut_groups_device: cw_sw_cut.h); both strands for them (cw_strand_run_device, cw_strand_run, cw_revcomp_device, cw_revcomp: cw_strand.h); reads placed on
 * their reference (cw_seed_run_device, cw_seed_run, cw_seed_spans_device, cw_seed_spans: cw_seed.h), or through an index of the whole reference
 * (cw_locate_build_device, cw_locate_run_device, cw_locate_run: cw_locate.h); the reads of a set that overlap each other (cw_overlap_count_device,
 * cw_overlap_build_device, cw_overlap_run_device, cw_overlap_run, cw_overlap_to_pile_device: cw_overlap.h).
 * What the operators' entry points share exists once, in the anonymous namespace: Layout (arrays 256-byte aligned in one allocation), locked (a _device entry
 * point is its run_*_locked body under the engine's mutex), dev_batch (cw_batch -> DevBatch), run_begin / run_end (the bracket round the stages of every run,
 * a window run's included) and HostTrip (a host form's round trip: lock, check_groups, the output layout, upload_groups, up / down / sync); each host form
 * states only its validation, its slots, its outputs, what else goes up, its device form and what it copies back.
 * The scratch plan is cw_plan.h (host arithmetic only); the host feeders, cw_window_positions among them, are cw_hostio.cpp.
 */
#include "cw_internal.h"
#include "cw_private.h"
#include "cw_device.h"
#include "cw_index.h"
#include "cw_chain.h"
#include "cw_poa.h"
#include "cw_poa_q.h"
#include "cw_finish.h"
#include "cw_extract.h"
#include "cw_stitch.h"
#include "cw_pack.h"
#include "cw_plan.h"
#include "cw_poa_op.h"
#include "cw_sw_op.h"
#include "cw_sw_path.h"
#include "cw_pileup.h"
#include "cw_sw_cut.h"
#include "cw_strand.h"
#include "cw_seed.h"
#include "cw_locate.h"
#include "cw_overlap.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <utility>
#include <vector>

namespace {

/* LDS budget of the POA tiers (160 KiB per CU): the occupancy the tier table of DESIGN.md states depends on these sums */
static_assert(4 * CW_POA_WAVES * CW_POA_SLAB_BYTES <= 163840, "tier S: at least four work-groups per CU (five under the default policy)");
static_assert(4 * CW_POAM1_WAVES * CW_POA_HOT2C_BYTES(CW_POAM1_NC, CW_POAM1_EC, CW_POAM1_LC) <= 163840, "tier M1: four work-groups per CU");
static_assert(4 * CW_POAM2_WAVES * CW_POA_HOT2T_BYTES(2, CW_POAM2_NC, CW_POAM2_EC, CW_POAM2_LC) <= 163840 || CW_M2_CODES, "tier M2: four work-groups per CU");
static_assert(CW_POAL_LDS_BYTES <= 40960, "tier L: a work-group fits the hole an M1/M2 work-group leaves");
static_assert(CW_IDX_STAGE_OFF + 16 + CW_IDX_STAGE_N * 8 + 4 * CW_IDX_STAGE_WORDS <= CW_IDX_LDS_BYTES, "index kernel: stage area inside the LDS allocation");

static_assert(CW_FIN_CB_BIG == CW_CONS_SLOT_MAX, "the largest consensus slot (include/consent_amd.h CW_CONS_SLOT_BYTES, engine.py cons_slot_bytes) is what the finish kernel's second pass holds");

/* ---- launch table: the dynamic LDS of every kernel that asks for some -- a constant, or a function of the work-group's waves where a knob chooses them.
   set_kernel_attributes allows each kernel the most its launch can ask for, and the launch passes the same name. */
constexpr size_t kLdsIndex = CW_IDX_LDS_BYTES;
constexpr size_t lds_chain(size_t slab) { return CW_CH_WAVES * slab; } /* CW_CH_SLAB, or CW_CH_SLAB_LONG for an engine configured for long templates */
constexpr size_t kLdsTierS = (size_t)CW_POA_SLAB_BYTES * CW_POA_WAVES;
constexpr size_t lds_tier_q(uint32_t waves) { return (size_t)CW_POAQ_TASK_BYTES * 4 * waves; } /* four tasks per wave */
constexpr size_t lds_tier_h(uint32_t waves) { return (size_t)CW_POAH_TASK_BYTES * 2 * waves; } /* two tasks per wave; six waves at most: cw_poa_h_kernel's launch bounds */
constexpr size_t kLdsFinish = (size_t)CW_FIN_SLAB * CW_FIN_WAVES, kLdsFinishBig = CW_FIN_SLAB_OF(0);
constexpr size_t kLdsStitch = (size_t)CW_ST_WAVES * CW_ST_SLAB; /* what the wide re-assembly kernel needs (it is given more: stitch_lds_one) */
constexpr size_t lds_sw(int cls) { return (size_t)CW_SW_WAVES * (cls == 0 ? CW_SW_SLAB_OF(CW_SW_Q0) : CW_SW_SLAB_OF(CW_ST_QMAX)); } /* the alignment operator's two LDS instances */
static_assert(4 * lds_sw(0) <= 163840, "cw_sw_kernel<0>: the four work-groups a CU its 128 registers allow");
constexpr size_t kLdsStrandWide = (size_t)CW_STR_SLOTS_WIDE * 4; /* the strand vote's wide table (the narrow one is static) */
constexpr size_t kLdsSeedWide = (size_t)CW_SEED_LDS_WORDS(CW_STR_SLOTS_WIDE, CW_SW_RMAX, CW_SEED_THREADS_WIDE) * 4; /* the seed run's wide table, reference words and histograms (the narrow ones are static) */

/* tiers M1, M2 and L are instances of cw_poa_slab_kernel: a tier's template arguments and the LDS of its work-group, PASS 0 = its own list, 1 = the overflow pass */
template <int NC, int EC, int LC, int WAVES, int TIER, size_t LDS>
struct SlabTier {
    static constexpr size_t lds = LDS;
    template <int PASS> static const void* kernel() { return (const void*)cw_poa_slab_kernel<NC, EC, LC, WAVES, TIER, PASS>; }
    template <int PASS> static void launch(uint32_t grid, hipStream_t st, const DevBatch& db, const DevScratch& sc) { cw_poa_slab_kernel<NC, EC, LC, WAVES, TIER, PASS><<<grid, 64 * WAVES, LDS, st>>>(db, sc); }
};
using TierM1 = SlabTier<CW_POAM1_NC, CW_POAM1_EC, CW_POAM1_LC, CW_POAM1_WAVES, 1, (size_t)CW_POA_HOT2C_BYTES(CW_POAM1_NC, CW_POAM1_EC, CW_POAM1_LC) * CW_POAM1_WAVES>;
using TierM2 = SlabTier<CW_POAM2_NC, CW_POAM2_EC, CW_POAM2_LC, CW_POAM2_WAVES, 2, (size_t)CW_POA_HOT2T_BYTES(2, CW_POAM2_NC, CW_POAM2_EC, CW_POAM2_LC) * CW_POAM2_WAVES>;
using TierL = SlabTier<CW_POAL_NC, CW_POAL_EC, CW_POAL_LC, CW_POAL_WAVES, 3, (size_t)CW_POAL_LDS_BYTES>;

int ensure(void** ptr, size_t* have, size_t need) {
    if (*have >= need) return CW_OK;
    if (*ptr) { if (hipFree(*ptr) != hipSuccess) return CW_E_NO_DEVICE; *ptr = nullptr; *have = 0; }
    /* a quarter more than asked for (bounded): hipFree + hipMalloc of a multi-gigabyte arena wait for the device and take up to seconds with a second
       engine at work on it, and the batches of a run differ by a few percent (the native driver's jobs: one regrowth instead of one per
       larger job -- the difference between 1.7 and 3-4 s for the E. coli-scale set) */
    size_t want = need + (need / 4 < ((size_t)1 << 30) ? need / 4 : ((size_t)1 << 30)); /* at most 1 GiB on top: several engines share a device */
    if (hipMalloc(ptr, want) != hipSuccess) {
        (void)hipGetLastError();
        want = need;
        if (hipMalloc(ptr, want) != hipSuccess) { *ptr = nullptr; return CW_E_NOMEM; }
    }
    *have = want;
    return CW_OK;
}

/* arrays laid one behind the other in one allocation, each 256-byte aligned: put returns where an array begins, bytes is what all of them take */
struct Layout {
    size_t bytes = 0;
    size_t put(size_t n) { const size_t at = bytes; bytes = align_up(bytes + n, 256); return at; }
};

/* an entry point that is `body` under the engine's mutex; a NULL engine is refused before the lock */
template <class F>
int locked(cw_engine* e, F body) {
    if (!e) return CW_E_INVALID;
    std::lock_guard<std::mutex> lk(e->mu);
    return body();
}

/* the batch as the kernels take it */
DevBatch dev_batch(const cw_batch* b) {
    DevBatch d;
    d.n_windows = b->n_windows; d.win_first_seq = b->win_first_seq; d.seq_len = b->seq_len; d.seq_word_off = b->seq_word_off; d.bases = b->bases;
    return d;
}

int check_params(const cw_params* p) {
    if (!p) return CW_E_INVALID;
    if (p->k < 2 || p->k > 16) return CW_E_INVALID; /* k-mers are 32-bit keys; k <= 9 counts in a direct LDS table, larger k in a hashed one */
    if (p->solid < 1 || p->max_msa < 1) return CW_E_INVALID;
    return CW_OK;
}

/* LDS request of the wide re-assembly kernel: what it needs, or -- to keep a second work-group off the CU (cw_stitch_device) -- a little more than
   half of what the DEVICE's CUs have (the constant 84 KB encoded gfx950's 160 KB), never more than a work-group may ask for */
size_t stitch_lds_one(const hipDeviceProp_t& prop) {
    size_t need = kLdsStitch, half = prop.sharedMemPerMultiprocessor / 2 + 4096, cap = prop.sharedMemPerBlock;
    if (prop.sharedMemPerMultiprocessor == 0) half = 84u * 1024u;
    size_t want = half > need ? half : need;
    if (cap >= need && want > cap) want = cap;
    return want;
}

int set_kernel_attributes(const hipDeviceProp_t& prop) {
    auto allow = [](const void* kernel, size_t lds) { return hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess; };
    const size_t lds_st = stitch_lds_one(prop);
    const bool ok = allow((const void*)cw_index_kernel, kLdsIndex) &&
        allow((const void*)cw_chain_kernel<CW_CH_SLAB>, lds_chain(CW_CH_SLAB)) && allow((const void*)cw_chain_kernel<CW_CH_SLAB_LONG>, lds_chain(CW_CH_SLAB_LONG)) &&
        allow((const void*)cw_poa_kernel, kLdsTierS) && allow((const void*)cw_poa_q_kernel, lds_tier_q(CW_POAQ_WAVES)) &&
#if CW_Q_CODES && defined(CW_TEST_AIDS) /* tier H: an opt-in kernel of the test-aid build (CW_TIER_H), not in the product's code object */
        allow((const void*)cw_poa_h_kernel, lds_tier_h(6)) &&
#endif
        allow(TierM1::kernel<0>(), TierM1::lds) && allow(TierM2::kernel<0>(), TierM2::lds) && allow(TierL::kernel<0>(), TierL::lds) &&
        allow(TierM1::kernel<1>(), TierM1::lds) && allow(TierM2::kernel<1>(), TierM2::lds) && allow(TierL::kernel<1>(), TierL::lds) &&
        allow((const void*)cw_finish_kernel<CW_FIN_CB, CW_FIN_WAVES, false>, kLdsFinish) && allow((const void*)cw_finish_kernel<CW_FIN_CB_BIG, 1, true>, kLdsFinishBig) &&
        allow((const void*)cw_stitch_kernel<CW_ST_QMAX, CW_ST_RMAX, 16, CW_ST_WAVES>, lds_st) &&
        allow((const void*)cw_sw_kernel<0, false>, lds_sw(0)) && allow((const void*)cw_sw_kernel<1, false>, lds_sw(1)) &&
        allow((const void*)cw_sw_path_kernel<0, false>, lds_sw(0)) && allow((const void*)cw_sw_path_kernel<1, false>, lds_sw(1)) &&
        allow((const void*)cw_pileup_kernel<0, false>, lds_sw(0)) && allow((const void*)cw_pileup_kernel<1, false>, lds_sw(1)) &&
        allow((const void*)cw_sw_cut_kernel<0, false>, lds_sw(0)) && allow((const void*)cw_sw_cut_kernel<1, false>, lds_sw(1)) &&
        allow((const void*)cw_sw_kernel<0, true>, lds_sw(0)) && allow((const void*)cw_sw_kernel<1, true>, lds_sw(1)) &&
        allow((const void*)cw_sw_path_kernel<0, true>, lds_sw(0)) && allow((const void*)cw_sw_path_kernel<1, true>, lds_sw(1)) &&
        allow((const void*)cw_pileup_kernel<0, true>, lds_sw(0)) && allow((const void*)cw_pileup_kernel<1, true>, lds_sw(1)) &&
        allow((const void*)cw_sw_cut_kernel<0, true>, lds_sw(0)) && allow((const void*)cw_sw_cut_kernel<1, true>, lds_sw(1)) &&
        allow((const void*)cw_strand_kernel<1>, kLdsStrandWide) && allow((const void*)cw_seed_kernel<1>, kLdsSeedWide);
    return ok ? CW_OK : CW_E_NO_DEVICE;
}

/* one named stage of a run: what `launch` enqueues on st, between the two events cw_last_timings and cw_poll read */
template <class L>
void stage(cw_engine* e, hipStream_t st, const char* name, L launch) {
    const int i = e->n_stages < CW_MAX_STAGES ? e->n_stages++ : CW_MAX_STAGES - 1;
    e->stage_name[i] = name;
    (void)hipEventRecord(e->ev0[i], st);
    launch();
    (void)hipEventRecord(e->ev1[i], st);
}

/* The bracket round the stages of every run: no stage recorded and ev_begin on st before them; ev_end, a look at the launches' errors and valid timings behind
   them.  takes_scratch: the run puts a plan of its own over the engine's scratch, which then no longer holds a window or POA run's records -- the inspection
   entry points and the re-run loop's look at the last run refuse (cw_debug_win_info, cw_debug_solid_table) or find nothing to do (grow_if_that_helps,
   decay_scale).  A window or POA run has noted its windows by then (hold_and_bind); the reverse complement and the seed spans use no scratch: all three pass
   false. */
int run_begin(cw_engine* e, hipStream_t st, bool takes_scratch) {
    if (takes_scratch) e->last_windows = 0;
    e->n_stages = 0;
    e->timings_valid = false;
    CW_HIP(hipEventRecord(e->ev_begin, st));
    return CW_OK;
}

int run_end(cw_engine* e, hipStream_t st) {
    CW_HIP(hipEventRecord(e->ev_end, st));
    CW_HIP(hipGetLastError());
    e->timings_valid = true;
    return CW_OK;
}

/* what a plan of this engine is made from, for a batch of these totals: its parameters, its device, the tier-G slots of its last run, its current scale and
   template length, the matrix slot by the mean depth.  Callers change what they ask about (a scale to try, pf_full). */
PlanInput plan_input(const cw_engine* e, uint32_t n_windows, uint32_t n_seqs, uint64_t n_words) { return PlanInput{e->prm, n_windows, n_seqs, n_words, e->cus, e->last_big_slots ? e->last_big_slots : 64u, e->cap_scale, e->tmax_plan, false}; }

/* The last run's BatchCounters in scratch: `bytes` of them from `off`, by an asynchronous copy on st into dst -- pinned: cw_host_fb -- and a wait for st:
   hipMemcpy's null stream would wait for every other stream of the device, the other worker's job among them.  The caller holds e->mu and has checked e->scratch. */
int read_counters(cw_engine* e, hipStream_t st, size_t off, size_t bytes, void* dst) {
    CW_HIP(hipSetDevice(e->device));
    CW_HIP(hipMemcpyAsync(dst, (const uint8_t*)e->scratch + e->last_ctr_off + off, bytes, hipMemcpyDeviceToHost, st)); CW_HIP(hipStreamSynchronize(st));
    return CW_OK;
}
int read_counters_idle(cw_engine* e, BatchCounters* c) { /* all of them, once everything on the device has ended: the inspection entry points */
    CW_HIP(hipSetDevice(e->device));
    CW_HIP(hipDeviceSynchronize());
    CW_HIP(hipMemcpy(c, (const uint8_t*)e->scratch + e->last_ctr_off, sizeof(*c), hipMemcpyDeviceToHost));
    return CW_OK;
}

/* ---- one device run: validate, plan and bind, launch shape, enqueue ----------------------------------------------------------- */

/* CW_OK for a batch that can run -- and for an empty one, which the caller answers without running */
int validate_run(const cw_engine* e, const cw_batch* batch, const cw_result* res) {
    if (!e || !batch || !res || !res->cons || !res->cons_off || !res->cons_len || !res->win_status) return CW_E_INVALID;
    if ((res->solid != nullptr) != (res->solid_off != nullptr) || (res->solid != nullptr) != (res->solid_len != nullptr)) return CW_E_INVALID;
    if (batch->n_windows == 0) return CW_OK;
    if (!batch->win_first_seq || !batch->seq_len || !batch->seq_word_off || !batch->bases) return CW_E_INVALID;
    /* per-window offsets into the arena, the solid table and the segment table are 32-bit (WinInfo, PoaTask): a batch is
       limited so that none of them can wrap -- split larger inputs (the library's own drivers do; cw_max_batch_windows) */
    if (batch->n_windows > max_batch_windows(e->tmax_plan)) return CW_E_INVALID;
    return CW_OK;
}

/* every pointer and capacity of DevScratch that comes from the plan; what depends on the batch and the knobs is launch_shape's */
DevScratch bind_scratch(const ScratchPlan& p, uint8_t* base) {
    DevScratch sc;
    memset(&sc, 0, sizeof(sc));
    sc.win = (WinInfo*)(base + p.win);
    sc.solid_key = (uint32_t*)(base + p.solid_key); sc.solid_cnt = (uint32_t*)(base + p.solid_cnt);
    sc.seg_off = (uint32_t*)(base + p.seg_off); sc.seg_len = (uint32_t*)(base + p.seg_len);
    sc.arena = base + p.arena;
    sc.tasks = (PoaTask*)(base + p.tasks); sc.task_cap = p.task_cap;
    sc.members = (PoaMember*)(base + p.members); sc.member_cap = p.member_cap;
    sc.ctr = (BatchCounters*)(base + p.ctr);
    sc.list_cap = p.task_cap;
    sc.list_cls = p.task_cap <= CW_LIST_IDX_MASK ? 1u : 0u; /* the neutral entry, task_cap itself, has to fit under the class byte too */
    for (int t = 0; t < CW_TIERS; ++t) {
        sc.tier_list[t] = (uint32_t*)(base + p.list[t]); sc.over_list[t] = (uint32_t*)(base + p.over[t]);
        sc.slab[t] = base + p.slab[t]; sc.slab_bytes[t] = p.tier[t].slab_bytes; sc.slots[t] = p.tier[t].slots;
        sc.slot_busy[t] = (uint32_t*)(base + p.sbusy[t]);
    }
    sc.q_slab = base + p.qslab; sc.h_slab = base + p.hslab;
    sc.p_fallback = (uint16_t*)(base + p.pfall); sc.p_fallback_elems = p.pfall_elems;
    sc.ablock = base + p.ablock; sc.ablock_units = p.ablock_units;
    sc.ex_fallback = (unsigned long long*)(base + p.exg);
    sc.task_dbg = getenv("CW_TASK_TRACE") ? (uint4*)(base + p.tdbg) : nullptr; /* (the plan gives it room under the same condition) */
    sc.fin_vis = (uint32_t*)(base + p.finvis); sc.fin_vis_words = CW_FIN_VIS_GLB_WORDS;
    sc.fin_retry = (uint32_t*)(base + p.finretry); sc.fin_big = base + p.finbig;
    return sc;
}

/* tier G's slabs at most, for the plans of both run shapes */
uint32_t plan_big_slots() {
    uint32_t big_slots = 64; /* tier G's kernel is sixteen work-groups of four waves at most (big_wgs, launch_shape): 64 slabs of 16.8 MB are all it can use (256 through round 5: 4.3 GB) */
    if (const char* env = CW_AID_ENV("CW_BIG_SLOTS")) { int v = atoi(env); if (v >= 4 && v <= 4096) big_slots = (uint32_t)v / 4 * 4; }
    return big_slots;
}

/* a plan of either run shape (plan_scratch, plan_poa): refuse it beyond the 32-bit offsets, see that the engine holds that much, bind it; remembers what the
   inspection entry points and the re-run loop need */
int hold_and_bind(cw_engine* e, uint32_t n_windows, uint32_t big_slots, const ScratchPlan& p, DevScratch* sc) {
    if (p.solid_cap > 0xFFFFFFFFull || p.seg_cap > 0xFFFFFFFFull || p.arena_cap > 0xFFFFFFFFull) return CW_E_INVALID; /* see CW_MAX_BATCH_WINDOWS */
    e->last_windows = n_windows; e->last_big_slots = big_slots; e->last_ctr_off = p.ctr;
    if (int rc = ensure(&e->scratch, &e->scratch_bytes, p.total)) return rc;
    e->last_tasks_off = p.tasks; e->last_tdbg_off = p.tdbg; e->last_task_cap = p.task_cap;
    e->last_solid_key_off = p.solid_key; e->last_solid_cnt_off = p.solid_cnt;
    e->last_seg_len_off = p.seg_len; e->last_members_off = p.members;
    static_assert(CW_TIERS == 6, "cw_engine::last_list_off");
    for (int t = 0; t < CW_TIERS; ++t) e->last_list_off[t] = p.list[t];
    e->last_ablock_off = p.ablock; e->last_ablock_units = p.ablock_units;
    if (!e->step_clock) { CW_HIP(hipMalloc((void**)&e->step_clock, 16)); CW_HIP(hipMemset(e->step_clock, 0, 16)); }
    *sc = bind_scratch(p, (uint8_t*)e->scratch);
    sc->step_clock = e->step_clock;
    return CW_OK;
}

/* plan the batch's scratch (cw_plan.h), hold it, bind it */
int plan_and_bind(cw_engine* e, const cw_batch* batch, bool pf_full, ScratchPlan* plan, DevScratch* sc) {
    const uint32_t big_slots = plan_big_slots();
    PlanInput in = plan_input(e, batch->n_windows, batch->n_seqs, batch->n_words);
    in.big_slots = big_slots; in.pf_full = pf_full;
    const ScratchPlan& p = *plan = plan_scratch(in);
    return hold_and_bind(e, batch->n_windows, big_slots, p, sc);
}

/* grids and work-group shapes of one run, but for the tier kernels' grids: those are DevScratch::persist_wgs, with the routing margins and the linger count */
struct LaunchShape {
    uint32_t h_waves, q_grid, q_waves, sort_lds, sort_thr, pass1_wgs, big_wgs, arena_div, no_tier_x; /* (pass1_wgs, big_wgs: the overflow pass -- tier L's second launch, tier G) */
};

uint32_t knob_u(const char* name, uint32_t dflt, uint32_t lo, uint32_t hi) { const char* v = CW_AID_ENV(name); if (!v) return dflt; const long x = atol(v); return x >= (long)lo && x <= (long)hi ? (uint32_t)x : dflt; }

/* what depends on the batch and the knobs: the grids, and in sc the routing margins, the tiers in use and the linger count */
LaunchShape launch_shape(cw_engine* e, const cw_batch* batch, const ScratchPlan& p, DevScratch& sc) {
    LaunchShape ls;
    const uint32_t cus = (uint32_t)e->cus, W = batch->n_windows;
    /* how many tier-L work-groups stay on the live overflow queue: about half of what the last finished batch handed over (few when
       nothing overflows, since a lingering work-group holds LDS the other tiers could use).  The count arrives in pinned host memory
       by an asynchronous copy at the end of each run: nothing here waits for the device */
    if (e->timings_valid) { /* a run has been enqueued before: its count, or that of the one before it, is there */
        const uint32_t want = e->host_fb->handed_over / 2;
        e->linger_wgs = want < 16 ? 16 : want > 256 ? 256 : want;
    }
    sc.linger_wgs = e->linger_wgs ? e->linger_wgs : 64;
    if (const char* env = CW_AID_ENV("CW_LINGER_WGS")) { int v = atoi(env); if (v >= 0 && v <= 1024) sc.linger_wgs = (uint32_t)v; }
    /* grids of the four concurrent tier kernels: every work-group loops until its tier's list is empty (sc.persist_wgs: see cw_poa_slab_kernel; none for tier G) */
    const TierMix mix = tier_mix();
    sc.persist_wgs[0] = tier_wgs_cap(0, W, cus * mix.s); sc.persist_wgs[1] = tier_wgs_cap(1, W, cus * mix.m1);
    sc.persist_wgs[2] = tier_wgs_cap(2, W, cus * mix.m2); sc.persist_wgs[3] = tier_wgs_cap(3, W, cus * mix.l);
    /* Tier H (two tasks per wave on 32-lane halves, cw_poa_q.h; round 5: tier Q's code instantiated for members of up to 63 bases and graphs of up
       to 128 nodes -- byte-sized graph arrays, recorded decisions, code words in the task's slab; it replaces round 3's opt-in kernel).  Bit-identical
       (tests/test_gpu_tier_q.py, test_gpu_parity.py) and OFF: measured on one box at depth 150 it takes tier S's 41.7 k tasks in 27.4 ms where tier
       S needs 28.4 -- 64 G wave-cycles against 69 -- and with its 18 waves per CU the other tiers slow down (M2 30.8 -> 36.7, L 41 -> 44 ms): step
       61-63 ms against 55-58; depth 30: 23.6 against 22.7.  Four tasks per wave (tier Q) beat tier S's scalar-controlled row loop six to one in
       machine time; two per wave do not: a per-lane row loop is ~100 instructions, tier S's 45.  CW_TIER_H=1|2 (test-aid build) turns it on. */
    /* Routing margins against late hand-overs.  A task that outgrows tier S or M1 is redone in tier L, whose work-groups only turn to the
       hand-over queue once their own list is empty: measured on a depth-150 batch (tools/task_trace.py), the ~150 tasks of 24-45 members
       x 27-31 bases that the depth-aware estimate put just inside tier S's 2048 cells, and the ~45 tasks of 52-64 members x 90-120 bases
       that outgrew tier M1's 256 nodes, kept a handful of tier-L waves busy for 10-20 ms after every other tier had finished.  With tier S
       taking only what is expected to stay below 1700 cells and tier M1 chosen by the depth-aware estimate as well, one task per batch is
       handed over instead of ~195, and the step (two engines) goes from 73.1 to 68.8 ms on the same box.  CW_S_ROUTE_CELLS /
       CW_M1_ROUTE_DEPTH=0 give the old routing (experiments; results do not depend on the tier). */
    sc.s_route_cells = 112; /* round 4: tier S has no cell limit any more; it takes a task whose graph is expected to stay below this many NODES (its capacity: CW_POA_NC) */
    if (const char* env = CW_AID_ENV("CW_S_ROUTE_NODES")) { const int v = atoi(env); if (v >= 8 && v <= CW_POA_NC) sc.s_route_cells = (uint32_t)v; }
    sc.m1_route_depth = 1u;
    if (const char* env = CW_AID_ENV("CW_M1_ROUTE_DEPTH")) sc.m1_route_depth = (uint32_t)atoi(env);
    sc.use_h = 0u; sc.h_min_len = CW_POAH_MIN_LEN;
    if (const char* env = CW_AID_ENV("CW_TIER_H")) { const int v = atoi(env); if (v >= 0 && v <= 2 && CW_Q_CODES) sc.use_h = (uint32_t)v; }
    if (const char* env = CW_AID_ENV("CW_H_MIN_LEN")) { const int v = atoi(env); if (v >= 1 && v <= CW_POAH_LC) sc.h_min_len = (uint32_t)v; }
    const uint32_t lds_cu = e->prop.sharedMemPerMultiprocessor ? (uint32_t)e->prop.sharedMemPerMultiprocessor : 160u * 1024u;
    auto wgs_lds_fit = [&](size_t lds) { return lds_cu / (((uint32_t)lds + 1023u) / 1024u * 1024u); }; /* work-groups whose LDS a CU holds (allocation granule: at most 1 KB) */
    ls.h_waves = 3; /* waves per tier-H work-group (two tasks per wave) */
    if (sc.use_h) {
        const uint32_t fit = wgs_lds_fit(lds_tier_h(ls.h_waves));
        uint32_t per_cu = fit < CW_POAH_WAVES / ls.h_waves ? (fit ? fit : 1u) : CW_POAH_WAVES / ls.h_waves;
        if (const char* env = CW_AID_ENV("CW_WGS_H")) { const int v = atoi(env); if (v >= 1 && (uint32_t)v <= per_cu) per_cu = (uint32_t)v; }
        sc.persist_wgs[5] = cus * per_cu;
    }
    const uint32_t* wgs = sc.persist_wgs;
    sc.producer_wgs = wgs[0] + wgs[1] + wgs[2] + wgs[5];
    if (CW_AID_ENV("CW_DEBUG_DONE")) fprintf(stderr, "[debug] producer_wgs %u = S %u + M1 %u + M2 %u, L %u, linger %u\n", sc.producer_wgs, wgs[0], wgs[1], wgs[2], wgs[3], sc.linger_wgs);
    sc.use_q = (CW_AID_ENV("CW_NO_TIER_Q") || CW_POA_AFFINE) ? 0u : 1u; /* (the affine gap model runs in the global-memory tier only: cw_poa_a.h) */
    /* Launch shapes chosen for two batches in flight on one GPU (two engines, or the driver's two workers): while the other batch's
       persistent tier kernels hold the LDS of every CU, a work-group that needs most of a CU waits for tens of milliseconds in the
       middle of this batch's chain (rocprofv3 timeline, depth 150: tier sort 0.45 -> 13-34 ms, tier Q 8.7 -> 55-94 ms with tier S
       queued behind it, the two overflow passes 0.05 -> 12-32 ms).  So: the sort is a small work-group (and since the classes
       travel in the list entries it keeps none of them in LDS: 17 KB of counters, static), tier Q runs as two-wave work-groups (38 KB; the same 8 waves per CU when it has the machine to itself),
       and the overflow passes -- normally a handful of tasks -- are 64 / 16 work-groups instead of two per CU.  Alone on the GPU the
       step time is unchanged. */
    ls.sort_lds = 0; /* no dynamic LDS: the class cache went when the classes moved into the list entries (cw_poa.h cw_list_entry) */
    ls.sort_thr = knob_u("CW_SORT_THREADS", 256, 128, 1024) / 64 * 64;
    ls.q_waves = knob_u("CW_Q_WAVES", CW_POAQ_WAVES % 3 == 0 ? 3 : CW_POAQ_WAVES % 2 == 0 ? 2 : 1, 1, CW_POAQ_WAVES); /* waves per tier-Q work-group (four tasks per wave; round 5: three-wave work-groups of 40 KB, four per CU) */
    const uint32_t q_fit = wgs_lds_fit(lds_tier_q(ls.q_waves));
    const uint32_t q_most = q_fit < CW_POAQ_WAVES / ls.q_waves ? (q_fit ? q_fit : 1u) : CW_POAQ_WAVES / ls.q_waves;
    ls.q_grid = cus * knob_u("CW_Q_WGS_PER_CU", q_most, 1, q_most);
    const uint32_t pass1_most = 64u < cus * 2u ? 64u : cus * 2u;
    ls.pass1_wgs = knob_u("CW_PASS1_WGS", pass1_most, 1, pass1_most);
    const uint32_t big_cap = p.tier[4].slots / CW_POA_WAVES;
    ls.big_wgs = knob_u("CW_BIG_WGS", big_cap < 16 ? big_cap : 16, 1, big_cap);
    ls.arena_div = 1; /* test aid: every window's arena slice divided, so that an ordinary window stops on it at x1 (CW_WHY_ARENA) */
    if (const char* env = CW_AID_ENV("CW_ARENA_DIV")) { const int v = atoi(env); if (v >= 2 && v <= 4096) ls.arena_div = (uint32_t)v; }
    ls.no_tier_x = CW_AID_ENV("CW_NO_TIER_X") ? 1 : 0;
    return ls;
}

/* what every run starts from: no stage recorded, the batch counters at zero, every slab free, tier L's live queue empty */
int enqueue_begin(cw_engine* e, hipStream_t st, const DevScratch& sc, const ScratchPlan& p) {
    if (sc.task_dbg) CW_HIP(hipMemsetAsync(sc.task_dbg, 0, (size_t)p.task_cap * 16, st)); /* (before ev_begin: not part of the run's time) */
    if (int rc = run_begin(e, st, false)) return rc;
    CW_HIP(hipMemsetAsync(sc.ctr, 0, sizeof(BatchCounters), st));
    CW_HIP(hipMemsetAsync(sc.slot_busy[0], 0, p.sbusy[CW_TIERS - 1] + (size_t)p.tier[CW_TIERS - 1].slots * 4 - p.sbusy[0], st)); /* every slab free */
    CW_HIP(hipMemsetAsync(sc.over_list[3], 0xFF, (size_t)p.task_cap * 4, st)); /* live queue: an entry is its own flag */
    return CW_OK;
}

/* ... and ends with: the feedback for the next batch's linger_wgs (pinned destination: asynchronous) */
int enqueue_end(cw_engine* e, hipStream_t st, const DevScratch& sc) {
    CW_HIP(hipMemcpyAsync(&e->host_fb->handed_over, &sc.ctr->n_over[3], 4, hipMemcpyDeviceToHost, st));
    return run_end(e, st);
}

/* The POA stage of a run, window or POA-only: sort, fork; tiers L / M2 / M1 on the side streams and Q (H) S on the engine's own, all concurrently; join; the
   overflow pass (L, G, X).  It depends on what comes before it only through tasks[], members[], the tier lists and seg_off / seg_len / arena. */
int enqueue_poa_stage(cw_engine* e, hipStream_t st, const DevBatch& db, const DevScratch& sc, const LaunchShape& ls) {
    const uint32_t* wgs = sc.persist_wgs;
    e->emitted_cap = 0;
    if (CW_AID_ENV("CW_KEEP_EMITTED")) { /* test aid: the lists as emitted, class bytes and all (cw_debug_tier_lists) */
        if (int rc = ensure(&e->emitted, &e->emitted_bytes, (size_t)CW_TIERS * sc.task_cap * 4)) return rc;
        for (int t = 0; t < CW_TIERS; ++t) CW_HIP(hipMemcpyAsync((uint32_t*)e->emitted + (size_t)t * sc.task_cap, sc.tier_list[t], (size_t)sc.task_cap * 4, hipMemcpyDeviceToDevice, st));
        e->emitted_cap = sc.task_cap;
    }
    cw_sort_tier_kernel<<<5, ls.sort_thr, ls.sort_lds, st>>>(sc); /* tiers M1, M2 and L: largest tasks first; tiers Q and H: like with like */
    /* pass 0: every tier works through its own routed list, all four concurrently; the long-running large tiers are
       dispatched first so that their tail overlaps the bulk of the small tasks */
    CW_HIP(hipEventRecord(e->ev_fork, st));
    for (int i = 0; i < 3; ++i) CW_HIP(hipStreamWaitEvent(e->side[i], e->ev_fork, 0));
    /* tier L also consumes the live overflow queue; only sc.linger_wgs of its work-groups stay for that (far fewer than
       CUs, so they can never keep the producers they wait for off the machine) */
    stage(e, e->side[2], "poa_large", [&] { TierL::launch<0>(wgs[3], e->side[2], db, sc); });
    stage(e, e->side[1], "poa_m2", [&] { TierM2::launch<0>(wgs[2], e->side[1], db, sc); });
    stage(e, e->side[0], "poa_m1", [&] { TierM1::launch<0>(wgs[1], e->side[0], db, sc); });
    /* Tiers Q and S go on the ENGINE's stream, also when the caller brought its own: the runtime multiplexes streams onto a few hardware
       queues, and a caller's stream that shares a queue with tier L's stream would make tier S wait for tier L's kernel to end --
       whose last work-groups wait for tier S to sign off (measured in the native driver: 131 ms per job until the bounded wait ran out).
       The engine's four streams were created together and first. */
    hipStream_t ms = e->stream;
    if (ms != st) CW_HIP(hipStreamWaitEvent(ms, e->ev_fork, 0));
    stage(e, ms, "poa_q", [&] { cw_poa_q_kernel<<<ls.q_grid, 64 * ls.q_waves, lds_tier_q(ls.q_waves), ms>>>(db, sc); }); /* four tasks per wave */
#if CW_Q_CODES && defined(CW_TEST_AIDS)
    if (wgs[5]) /* two tasks per wave; hands what outgrows it to tier L's live queue, as tier S does */
        stage(e, ms, "poa_h", [&] { cw_poa_h_kernel<<<wgs[5], 64 * ls.h_waves, lds_tier_h(ls.h_waves), ms>>>(db, sc); });
#endif
    stage(e, ms, "poa", [&] { cw_poa_kernel<<<wgs[0], 64 * CW_POA_WAVES, kLdsTierS, ms>>>(db, sc); }); /* CW_POA_SLAB_BYTES (about 7.7 KB) per wave */
    if (ms != st) { CW_HIP(hipEventRecord(e->ev_join_s, ms)); CW_HIP(hipStreamWaitEvent(st, e->ev_join_s, 0)); }
    for (int i = 0; i < 3; ++i) { CW_HIP(hipEventRecord(e->ev_join[i], e->side[i])); CW_HIP(hipStreamWaitEvent(st, e->ev_join[i], 0)); }
    /* pass 1: tasks that outgrew their tier (normally a handful) go straight to tier L, and from there to G */
    stage(e, st, "poa_overflow", [&] {
        TierL::launch<1>(ls.pass1_wgs, st, db, sc);
        cw_poa_big_kernel<<<ls.big_wgs, 64 * CW_POA_WAVES, 0, st>>>(db, sc);
        cw_poa_x_kernel<<<1, 64, 0, st>>>(db, sc, ls.no_tier_x); /* what outgrew tier G, in its slab pool (ends at once when tier G handed nothing on) */
    });
    return CW_OK;
}

/* The order of a step: setup, index, chain, sort, fork; tiers L / M2 / M1 on the side streams and Q (H) S on the engine's own, all concurrently; join;
   the overflow pass (L, G, X), finish, the feedback copy.  The stage names and their order are what bench.py and cw_poll match on.  A tier's grid is
   its persist_wgs (launch_shape). */
int enqueue(cw_engine* e, hipStream_t st, const cw_batch* batch, const DevBatch& db, const DevScratch& sc, const ScratchPlan& p, const LaunchShape& ls, const FinOut& fo) {
    const uint32_t cus = (uint32_t)e->cus, W = batch->n_windows;
    if (int rc = enqueue_begin(e, st, sc, p)) return rc;
    stage(e, st, "setup", [&] {
        cw_setup_need_kernel<<<(W + 3) / 4, 256, 0, st>>>(db, sc, e->prm);
        cw_setup_kernel<<<1, 1024, 0, st>>>(db, sc, e->prm, p.solid_cap, p.seg_cap, p.arena_cap, p.arena_scale, e->tmax_plan, ls.arena_div);
    });
    stage(e, st, "index", [&] { cw_index_kernel<<<W < cus ? W : cus, CW_IDX_THREADS, kLdsIndex, st>>>(db, sc, e->prm); });
    stage(e, st, "chain", [&] {
        const uint32_t want = (W + CW_CH_WAVES - 1) / CW_CH_WAVES;
        const uint32_t cap = cus * 2u; /* 2 work-groups x 4 waves x 20 KiB per CU */
        if (e->tmax_plan > 1024u) /* an engine configured for long templates (cw_configure): 32 KiB per wave, up to CW_TMAX anchors, one work-group per CU */
            cw_chain_kernel<CW_CH_SLAB_LONG><<<want < cus ? want : cus, 64 * CW_CH_WAVES, lds_chain(CW_CH_SLAB_LONG), st>>>(db, sc, e->prm);
        else
            cw_chain_kernel<CW_CH_SLAB><<<want < cap ? want : cap, 64 * CW_CH_WAVES, lds_chain(CW_CH_SLAB), st>>>(db, sc, e->prm);
    });
    if (int rc = enqueue_poa_stage(e, st, db, sc, ls)) return rc;
    stage(e, st, "finish", [&] {
        uint32_t grid = (W + CW_FIN_WAVES - 1) / CW_FIN_WAVES;
        if (grid > cus * CW_FIN_WGS_PER_CU) grid = cus * CW_FIN_WGS_PER_CU;
        cw_finish_kernel<CW_FIN_CB, CW_FIN_WAVES, false><<<grid, 64 * CW_FIN_WAVES, kLdsFinish, st>>>(db, sc, e->prm, fo);
        /* second pass: the windows whose strings outgrew the first pass's buffers (normally none: the kernel reads one counter and ends) */
        cw_finish_kernel<CW_FIN_CB_BIG, 1, true><<<W < 64u ? W : 64u, 64, kLdsFinishBig, st>>>(db, sc, e->prm, fo);
    });
    return enqueue_end(e, st, sc);
}

/* the body of cw_run_device; the caller holds e->mu */
/* pf_full: the index kernel's global matrix slot at its full kPfRowsMax rows (a re-run after CW_WHY_MATRIX, grow_if_that_helps) */
int run_device_locked(cw_engine* e, const cw_batch* batch, const cw_result* res, void* hip_stream, bool pf_full = false) {
    int rc = validate_run(e, batch, res);
    if (rc || batch->n_windows == 0) return rc;
    CW_HIP(hipSetDevice(e->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : e->stream;
    ScratchPlan p; DevScratch sc;
    if ((rc = plan_and_bind(e, batch, pf_full, &p, &sc)) != CW_OK) return rc;
    const LaunchShape ls = launch_shape(e, batch, p, sc);
    const DevBatch db = dev_batch(batch);
    e->last_win_first_seq = batch->win_first_seq;
    FinOut fo;
    fo.cons = res->cons; fo.cons_off = res->cons_off; fo.cons_len = res->cons_len; fo.win_status = res->win_status;
    fo.solid = res->solid; fo.solid_off = res->solid_off; fo.solid_len = res->solid_len;
    return enqueue(e, st, batch, db, sc, p, ls, fo);
}

/* CW_OK for a batch of groups that can run -- and for an empty one; nothing here touches the device */
int validate_poa(const cw_engine* e, const cw_batch* groups, const cw_result* res) {
    if (!e || !groups || !res || !res->cons || !res->cons_off || !res->cons_len || !res->win_status) return CW_E_INVALID;
    if (res->solid || res->solid_off || res->solid_len) return CW_E_INVALID; /* a group has no solid set */
    if (groups->n_windows == 0) return CW_OK;
    if (!groups->win_first_seq || !groups->seq_len || !groups->seq_word_off || !groups->bases) return CW_E_INVALID;
    if (groups->n_windows > max_batch_windows(e->tmax_plan)) return CW_E_INVALID; /* cw_max_batch_windows */
    if (plan_poa(groups->n_windows, groups->n_seqs, groups->n_words, 1, 64).arena_cap > 0xFFFFFFFFull) return CW_E_INVALID; /* the arena's 32-bit offsets */
    return CW_OK;
}

/* the body of cw_poa_run_device; the caller holds e->mu.  The order of such a run: poa_tasks, the POA stage of a window run, poa_gather. */
int poa_device_locked(cw_engine* e, const cw_batch* groups, const cw_result* res, void* hip_stream) {
    int rc = validate_poa(e, groups, res);
    if (rc || groups->n_windows == 0) return rc;
    CW_HIP(hipSetDevice(e->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : e->stream;
    const uint32_t G = groups->n_windows, big_slots = plan_big_slots();
    const ScratchPlan p = plan_poa(G, groups->n_seqs, groups->n_words, e->cus, big_slots); /* exact: no run with a larger plan follows */
    DevScratch sc;
    if ((rc = hold_and_bind(e, G, big_slots, p, &sc)) != CW_OK) return rc;
    const LaunchShape ls = launch_shape(e, groups, p, sc);
    const DevBatch db = dev_batch(groups);
    e->last_win_first_seq = groups->win_first_seq;
    PoaOut po;
    po.cons = res->cons; po.cons_off = res->cons_off; po.cons_len = res->cons_len; po.win_status = res->win_status;
    if ((rc = enqueue_begin(e, st, sc, p)) != CW_OK) return rc;
    const uint32_t grid = (G + CW_POAOP_WAVES - 1) / CW_POAOP_WAVES;
    stage(e, st, "poa_tasks", [&] { cw_poa_tasks_kernel<<<grid, 64 * CW_POAOP_WAVES, 0, st>>>(db, sc, e->prm.max_msa, groups->n_seqs, p.arena_cap); });
    if ((rc = enqueue_poa_stage(e, st, db, sc, ls)) != CW_OK) return rc;
    stage(e, st, "poa_gather", [&] { cw_poa_gather_kernel<<<grid, 64 * CW_POAOP_WAVES, 0, st>>>(db, sc, po); });
    return enqueue_end(e, st, sc);
}

/* ---- the alignment operator's four runs: cw_sw_run, cw_sw_path_run, cw_pileup_run, cw_sw_cut_run (and their _device forms) ------------------------------- */

/* What the four refuse alike, e and groups given: CW_OK for a batch of groups whose pairs can be aligned -- and for one without sequences, before a look at
   rows (the strand runs: their per-sequence output); nothing here touches the device.  Each validate_* below keeps its own checks and their place before or
   behind these. */
int validate_groups(const cw_engine* e, const cw_batch* groups, const void* rows) {
    if (groups->n_windows > max_batch_windows(e->tmax_plan)) return CW_E_INVALID; /* cw_max_batch_windows */
    if (groups->n_windows == 0 || groups->n_seqs == 0) return groups->n_seqs == 0 ? CW_OK : CW_E_INVALID; /* (sequences belong to groups) */
    if (!rows || !groups->win_first_seq || !groups->seq_len || !groups->seq_word_off || !groups->bases) return CW_E_INVALID;
    return CW_OK;
}

int validate_sw(const cw_engine* e, const cw_batch* groups, const int32_t* rows, uint32_t flags) {
    if (!e || !groups || (flags & ~CW_SW_WANT_INDELS)) return CW_E_INVALID;
    return validate_groups(e, groups, rows);
}

int validate_sw_path(const cw_engine* e, const cw_batch* groups, const int32_t* rows, const cw_sw_paths* paths, uint32_t flags) {
    if (!e || !groups || !paths || (flags & ~CW_SW_PATH_EQX)) return CW_E_INVALID;
    const int rc = validate_groups(e, groups, rows);
    if (rc || groups->n_seqs == 0) return rc;
    if (!paths->ops || !paths->ops_off || !paths->n_ops) return CW_E_INVALID;
    return CW_OK;
}

/* (the pileup and cut runs refuse a missing output for a batch without sequences too) */
int validate_pileup(const cw_engine* e, const cw_batch* groups, const int32_t* rows, const cw_pileup* pile, uint32_t flags) {
    if (!e || !groups || !pile || (flags & ~CW_PILE_ACCUMULATE)) return CW_E_INVALID;
    if (!rows || !pile->counts || !pile->col_off) return CW_E_INVALID;
    return validate_groups(e, groups, rows);
}

int validate_sw_cut(const cw_engine* e, const cw_batch* groups, const int32_t* rows, const cw_sw_cuts* cuts) {
    if (!e || !groups || !cuts) return CW_E_INVALID;
    if (!rows || !cuts->cuts || !cuts->cut_off || cuts->window == 0u) return CW_E_INVALID;
    return validate_groups(e, groups, rows);
}

/* What a span run (cw_sw_span_run and its kin) refuses on top of its counterpart, once the batch is known to hold sequences: a missing member.  spans is NULL
   for the entry points without spans; the span entry points refuse a NULL of their own before they come here. */
int validate_spans(const cw_sw_spans* spans, uint32_t n_seqs) {
    return spans && n_seqs > 0 && (!spans->ref_lo || !spans->ref_hi) ? CW_E_INVALID : CW_OK;
}

/* The device, the stream and the plan's bytes of a run.  The plan lives in the engine's one scratch allocation, like a window run's and a POA run's: runs on one
   engine are serialised by its mutex and ordered on its stream (or by the caller, include/consent_amd.h "Threading"), so none of them is in flight while
   another's plan is bound.  (stitch_scratch is cw_stitch_device's alone: nothing here touches it.) */
int hold_sw(cw_engine* e, size_t total, void* hip_stream, hipStream_t* st) {
    CW_HIP(hipSetDevice(e->device));
    *st = hip_stream ? (hipStream_t)hip_stream : e->stream;
    return ensure(&e->scratch, &e->scratch_bytes, total);
}

/* the arguments every kernel of the four runs takes, by the plan's offsets (a path plan is a plan and the steps) */
SwArgs bind_sw(const cw_engine* e, const cw_batch* groups, int32_t* rows, uint32_t flags, const SwPlan& p, const cw_sw_spans* spans) {
    uint8_t* base = (uint8_t*)e->scratch;
    SwArgs a;
    a.b = dev_batch(groups);
    a.n_seqs = groups->n_seqs; a.rows = rows; a.flags = flags;
    a.ctr = (uint32_t*)(base + p.ctr); a.seq_ref = (uint32_t*)(base + p.seq_ref); a.order = (uint32_t*)(base + p.order);
    a.dir = p.dir_bytes ? (int8_t*)(base + p.dir) : nullptr; a.dir_bytes = p.dir_bytes;
    a.gref = base + p.gref; a.lstate = base + p.lstate;
    a.ref_lo = spans ? spans->ref_lo : nullptr; a.ref_hi = spans ? spans->ref_hi : nullptr;
    return a;
}

/* a run's three alignment stages: their names and kernels, by query class */
template <class Args>
struct SwStages { const char* names[3]; void (*k0)(Args); void (*k1)(Args); void (*k_long)(Args); };

/* what one run or another adds around the order stage; all absent for the plain run */
struct SwExtras {
    uint32_t* zero = nullptr;       /* the path run: n_seqs words to clear behind the counters (n_ops: rows the order kernel writes, and pairs without a path) */
    const CutArgs* rest = nullptr;  /* the cut run: cw_sw_cut_rest_kernel inside the order stage */
    const PileArgs* clear = nullptr; /* the pileup run unless it accumulates: the pile_clear stage behind the order stage */
};

/* The order of a run: sw_order (three small launches, and the cut run's fourth), pile_clear when asked for, then the alignment launches by query class, one
   after the other on st: up to CW_SW_Q0 bases, up to CW_ST_QMAX, beyond (ends at once when there is no such pair; the order kernel's counts stay on the device,
   so nothing here waits for it). */
template <class Args>
int enqueue_sw_run(cw_engine* e, hipStream_t st, const SwArgs& a, const SwPlan& p, const SwStages<Args>& k, const Args& args, const SwExtras& x = SwExtras()) {
    if (int rc = run_begin(e, st, true)) return rc;
    CW_HIP(hipMemsetAsync(a.ctr, 0, (size_t)CW_SW_CTR_WORDS * 4, st));
    if (x.zero) CW_HIP(hipMemsetAsync(x.zero, 0, (size_t)a.n_seqs * 4, st));
    const uint32_t og = (a.n_seqs + 255u) / 256u;
    stage(e, st, "sw_order", [&] {
        cw_sw_order_kernel<<<og, 256, 0, st>>>(a, 0);
        cw_sw_order_kernel<<<1, 256, 0, st>>>(a, 1);
        cw_sw_order_kernel<<<og, 256, 0, st>>>(a, 2);
        if (x.rest) cw_sw_cut_rest_kernel<<<og, 256, 0, st>>>(*x.rest);
    });
    if (x.clear) stage(e, st, "pile_clear", [&] { cw_pileup_clear_kernel<<<a.b.n_windows, 256, 0, st>>>(*x.clear); });
    stage(e, st, k.names[0], [&] { k.k0<<<p.wgs0, 64 * CW_SW_WAVES, lds_sw(0), st>>>(args); });
    stage(e, st, k.names[1], [&] { k.k1<<<p.wgs1, 64 * CW_SW_WAVES, lds_sw(1), st>>>(args); });
    stage(e, st, k.names[2], [&] { k.k_long<<<p.wgs_long, 64, 0, st>>>(args); });
    return run_end(e, st);
}

/* the body of cw_sw_run_device and of cw_sw_span_run_device (spans: NULL for the first; the same in the three bodies below); the caller holds e->mu.  Stages: sw_order, sw_align, sw_align_wide, sw_align_long. */
int run_sw_locked(cw_engine* e, const cw_batch* groups, int32_t* rows, uint32_t flags, void* hip_stream, const cw_sw_spans* spans = nullptr) {
    int rc = validate_sw(e, groups, rows, flags);
    if (!rc) rc = validate_spans(spans, groups->n_seqs);
    if (rc || groups->n_seqs == 0) return rc;
    const SwPlan p = plan_sw(groups->n_windows, groups->n_seqs, groups->n_words, e->cus, flags); /* exact: no run with a larger plan follows */
    hipStream_t st;
    if ((rc = hold_sw(e, p.total, hip_stream, &st)) != CW_OK) return rc;
    const SwArgs a = bind_sw(e, groups, rows, flags, p, spans);
    return enqueue_sw_run(e, st, a, p, spans ? SwStages<SwArgs>{{"sw_align", "sw_align_wide", "sw_align_long"}, cw_sw_kernel<0, true>, cw_sw_kernel<1, true>, cw_sw_long_kernel<true>}
                                       : SwStages<SwArgs>{{"sw_align", "sw_align_wide", "sw_align_long"}, cw_sw_kernel<0, false>, cw_sw_kernel<1, false>, cw_sw_long_kernel<false>}, a);
}

/* the body of cw_sw_path_run_device.  Stages: sw_order, sw_path, sw_path_wide, sw_path_long. */
int run_sw_path_locked(cw_engine* e, const cw_batch* groups, int32_t* rows, const cw_sw_paths* paths, uint32_t flags, void* hip_stream, const cw_sw_spans* spans = nullptr) {
    int rc = validate_sw_path(e, groups, rows, paths, flags);
    if (!rc) rc = validate_spans(spans, groups->n_seqs);
    if (rc || groups->n_seqs == 0) return rc;
    const SwPathPlan p = plan_sw_path(groups->n_windows, groups->n_seqs, groups->n_words, e->cus);
    hipStream_t st;
    if ((rc = hold_sw(e, p.total, hip_stream, &st)) != CW_OK) return rc;
    SwPathArgs pa;
    pa.a = bind_sw(e, groups, rows, flags, p, spans);
    pa.ops = paths->ops; pa.ops_off = paths->ops_off; pa.n_ops = paths->n_ops; pa.steps = (uint8_t*)e->scratch + p.steps;
    SwExtras x;
    x.zero = pa.n_ops;
    return enqueue_sw_run(e, st, pa.a, p, spans ? SwStages<SwPathArgs>{{"sw_path", "sw_path_wide", "sw_path_long"}, cw_sw_path_kernel<0, true>, cw_sw_path_kernel<1, true>, cw_sw_path_long_kernel<true>}
                                       : SwStages<SwPathArgs>{{"sw_path", "sw_path_wide", "sw_path_long"}, cw_sw_path_kernel<0, false>, cw_sw_path_kernel<1, false>, cw_sw_path_long_kernel<false>}, pa, x);
}

/* the body of cw_pileup_run_device.  Stages: sw_order, pile_clear unless the run accumulates, pile, pile_wide, pile_long.  The plan is plan_sw_path's: there is
   no op memory to add. */
int run_pileup_locked(cw_engine* e, const cw_batch* groups, int32_t* rows, const cw_pileup* pile, uint32_t flags, void* hip_stream, const cw_sw_spans* spans = nullptr) {
    int rc = validate_pileup(e, groups, rows, pile, flags);
    if (!rc) rc = validate_spans(spans, groups->n_seqs);
    if (rc || groups->n_seqs == 0) return rc;
    if ((uintptr_t)pile->counts & 15u) return CW_E_INVALID; /* the clearing stores 16 bytes at a time */
    const SwPathPlan p = plan_sw_path(groups->n_windows, groups->n_seqs, groups->n_words, e->cus);
    hipStream_t st;
    if ((rc = hold_sw(e, p.total, hip_stream, &st)) != CW_OK) return rc;
    PileArgs pa;
    pa.a = bind_sw(e, groups, rows, flags, p, spans);
    pa.counts = pile->counts; pa.col_off = pile->col_off; pa.steps = (uint8_t*)e->scratch + p.steps;
    SwExtras x;
    if (!(flags & CW_PILE_ACCUMULATE)) x.clear = &pa;
    return enqueue_sw_run(e, st, pa.a, p, spans ? SwStages<PileArgs>{{"pile", "pile_wide", "pile_long"}, cw_pileup_kernel<0, true>, cw_pileup_kernel<1, true>, cw_pileup_long_kernel<true>}
                                       : SwStages<PileArgs>{{"pile", "pile_wide", "pile_long"}, cw_pileup_kernel<0, false>, cw_pileup_kernel<1, false>, cw_pileup_long_kernel<false>}, pa, x);
}

/* the body of cw_sw_cut_run_device.  Stages: sw_order -- with it the zeros of the queries that are no pair -- cut, cut_wide, cut_long.  The plan is
   plan_sw_path's. */
int run_sw_cut_locked(cw_engine* e, const cw_batch* groups, int32_t* rows, const cw_sw_cuts* cuts, void* hip_stream, const cw_sw_spans* spans = nullptr) {
    int rc = validate_sw_cut(e, groups, rows, cuts);
    if (!rc) rc = validate_spans(spans, groups->n_seqs);
    if (rc || groups->n_seqs == 0) return rc;
    const SwPathPlan p = plan_sw_path(groups->n_windows, groups->n_seqs, groups->n_words, e->cus);
    hipStream_t st;
    if ((rc = hold_sw(e, p.total, hip_stream, &st)) != CW_OK) return rc;
    CutArgs ca;
    ca.a = bind_sw(e, groups, rows, 0u, p, spans);
    ca.cuts = cuts->cuts; ca.cut_off = cuts->cut_off; ca.window = cuts->window; ca.steps = (uint8_t*)e->scratch + p.steps;
    SwExtras x;
    x.rest = &ca;
    return enqueue_sw_run(e, st, ca.a, p, spans ? SwStages<CutArgs>{{"cut", "cut_wide", "cut_long"}, cw_sw_cut_kernel<0, true>, cw_sw_cut_kernel<1, true>, cw_sw_cut_long_kernel<true>}
                                       : SwStages<CutArgs>{{"cut", "cut_wide", "cut_long"}, cw_sw_cut_kernel<0, false>, cw_sw_cut_kernel<1, false>, cw_sw_cut_long_kernel<false>}, ca, x);
}

/* ---- host buffers in, host buffers out: what cw_sw_run and the other host forms of the operators do alike ------------------------------------------------------ */

/* One synchronous call on host buffers, under the engine's mutex from its construction on: the device buffers are the engine's.  A host form validates (its
   own validate_*, which answers a batch without sequences before anything here), then: check_groups with its slot offsets if it has some; its outputs laid
   out in `out` and its own host allocations; upload_groups; up() of what else its run reads; its device form on `st` with `db`, dev_spans() and at() of its
   outputs; down() of what comes back; sync(); and the caller's bytes it owns written on the host.  Checks and host allocations, the two device buffers, then
   the uploads, then the run: behind the first enqueued copy a form returns early only when the runtime or the run itself fails. */
struct HostTrip {
    cw_engine* const e;
    const cw_batch* const b;
    const cw_sw_spans* const spans; /* a span form's two host arrays: they go up with the batch; NULL otherwise */
    std::lock_guard<std::mutex> lk;
    Layout out;                     /* the form's outputs, and what else it sends up, in e->poa_out */
    std::vector<uint64_t> slot;     /* check_groups: the slot offsets rebased to the first slot -- the device copy of the slots begins there; lives until sync() */
    cw_batch db;                    /* upload_groups: the batch with device pointers, */
    const uint64_t* d_slot = nullptr; /* `slot` on the device, */
    cw_sw_spans dsp;                /* the spans on the device (dev_spans()), */
    hipStream_t st = nullptr;       /* the engine's stream */
    uint8_t* dout = nullptr;        /* and e->poa_out, out.bytes of it */

    HostTrip(cw_engine* e_, const cw_batch* b_, const cw_sw_spans* spans_ = nullptr) : e(e_), b(b_), spans(spans_), lk(e_->mu) {}
    int check_groups(const uint64_t* slot_off);
    int upload_groups();
    const cw_sw_spans* dev_spans() const { return spans ? &dsp : nullptr; }
    template <class T> T* at(size_t off) const { return (T*)(dout + off); }
    hipError_t up(size_t off, const void* src, size_t bytes) { return bytes ? hipMemcpyAsync(dout + off, src, bytes, hipMemcpyHostToDevice, st) : hipSuccess; }
    hipError_t down(void* dst, size_t off, size_t bytes) { return bytes ? hipMemcpyAsync(dst, dout + off, bytes, hipMemcpyDeviceToHost, st) : hipSuccess; }
    hipError_t sync() { return hipStreamSynchronize(st); }
};

/* What the host forms check first: the groups begin at sequence 0, end at n_seqs and never step back, every sequence lies inside n_words, and the run's slot
   offsets slot_off[0 .. n_seqs], when it has some (else NULL), never step back. */
int HostTrip::check_groups(const uint64_t* slot_off) {
    const uint32_t G = b->n_windows, S = b->n_seqs;
    if (b->win_first_seq[0] != 0 || b->win_first_seq[G] != S) return CW_E_INVALID;
    for (uint32_t g = 0; g < G; ++g) if (b->win_first_seq[g + 1] < b->win_first_seq[g]) return CW_E_INVALID;
    for (uint32_t s = 0; s < S; ++s) {
        if (b->seq_word_off[s] + ((uint64_t)b->seq_len[s] + 15) / 16 > b->n_words) return CW_E_INVALID;
        if (slot_off && slot_off[s + 1] < slot_off[s]) return CW_E_INVALID;
    }
    if (slot_off) {
        try { slot.resize((size_t)S + 1); } catch (...) { return CW_E_NOMEM; }
        for (uint32_t s = 0; s <= S; ++s) slot[s] = slot_off[s] - slot_off[0];
    }
    return CW_OK;
}

/* the engine's two buffers for host forms, of at least these sizes, on its device: the hold step of every host form, cw_poa_run included */
int hold_io(cw_engine* e, size_t in_bytes, size_t out_bytes) {
    CW_HIP(hipSetDevice(e->device));
    if (int rc = ensure(&e->poa_in, &e->poa_in_bytes, in_bytes)) return rc;
    return ensure(&e->poa_out, &e->poa_out_bytes, out_bytes);
}

/* The checked batch goes up, on the engine's stream: into the engine's input buffer (the one cw_poa_run uses for its own), every array 256-byte aligned, behind
   it the rebased slot offsets when the form has slots, behind those a span form's two arrays.  The buffers are held here, both of them and before the first
   copy; a host form calls this last before its own uploads and the run, with its host allocations made and `out` laid out. */
int HostTrip::upload_groups() {
    const uint32_t G = b->n_windows, S = b->n_seqs;
    Layout in;
    const size_t i_wfs = in.put((size_t)(G + 1) * 4), i_len = in.put((size_t)S * 4), i_off = in.put((size_t)S * 8), i_bases = in.put((size_t)(b->n_words + 1) * 4),
                 i_slot = slot.empty() ? 0 : in.put((size_t)(S + 1) * 8), i_lo = spans ? in.put((size_t)S * 4) : 0, i_hi = spans ? in.put((size_t)S * 4) : 0;
    if (int rc = hold_io(e, in.bytes, out.bytes)) return rc;
    uint8_t* din = (uint8_t*)e->poa_in;
    dout = (uint8_t*)e->poa_out;
    st = e->stream;
    CW_HIP(hipMemcpyAsync(din + i_wfs, b->win_first_seq, (size_t)(G + 1) * 4, hipMemcpyHostToDevice, st));
    CW_HIP(hipMemcpyAsync(din + i_len, b->seq_len, (size_t)S * 4, hipMemcpyHostToDevice, st));
    CW_HIP(hipMemcpyAsync(din + i_off, b->seq_word_off, (size_t)S * 8, hipMemcpyHostToDevice, st));
    if (b->n_words) CW_HIP(hipMemcpyAsync(din + i_bases, b->bases, (size_t)b->n_words * 4, hipMemcpyHostToDevice, st));
    if (!slot.empty()) {
        CW_HIP(hipMemcpyAsync(din + i_slot, slot.data(), (size_t)(S + 1) * 8, hipMemcpyHostToDevice, st));
        d_slot = (const uint64_t*)(din + i_slot);
    }
    if (spans) {
        CW_HIP(hipMemcpyAsync(din + i_lo, spans->ref_lo, (size_t)S * 4, hipMemcpyHostToDevice, st));
        CW_HIP(hipMemcpyAsync(din + i_hi, spans->ref_hi, (size_t)S * 4, hipMemcpyHostToDevice, st));
        dsp.ref_lo = (const uint32_t*)(din + i_lo); dsp.ref_hi = (const uint32_t*)(din + i_hi);
    }
    db = *b;
    db.win_first_seq = (const uint32_t*)(din + i_wfs); db.seq_len = (const uint32_t*)(din + i_len);
    db.seq_word_off = (const uint64_t*)(din + i_off); db.bases = (const uint32_t*)(din + i_bases);
    return CW_OK;
}

/* what a host-buffer entry point answers for the rows that came back: CW_E_CAPACITY when a pair was beyond a capacity */
int sw_rows_rc(const int32_t* rows, uint32_t n_seqs) {
    for (uint32_t s = 0; s < n_seqs; ++s) if (rows[(size_t)s * CW_SW_ROW + CW_SW_STATUS] == CW_SW_STOP) return CW_E_CAPACITY;
    return CW_OK;
}

/* ---- both strands: cw_strand_run, cw_revcomp (and their _device forms) ------------------------------------------------------------------------------------- */

int validate_strand(const cw_engine* e, const cw_batch* groups, const cw_strands* out) {
    if (!e || !groups || !out || !out->strand) return CW_E_INVALID;
    if (out->k != 0u && (out->k < CW_STRAND_KMIN || out->k > CW_STRAND_KMAX)) return CW_E_INVALID;
    return validate_groups(e, groups, out->strand);
}

int validate_revcomp(const cw_engine* e, const cw_batch* groups, const uint32_t* bases_out) {
    if (!e || !groups || !bases_out || bases_out == groups->bases) return CW_E_INVALID;
    return validate_groups(e, groups, bases_out);
}

/* the body of cw_strand_run_device; the caller holds e->mu.  Stages: strand_order (the units of every group), strand (references of up to CW_ST_RMAX bases),
   strand_wide (beyond).  The plan lives in the engine's scratch, as an alignment run's. */
int run_strand_locked(cw_engine* e, const cw_batch* groups, const cw_strands* out, void* hip_stream) {
    int rc = validate_strand(e, groups, out);
    if (rc || groups->n_seqs == 0) return rc;
    const StrandPlan p = plan_strand(groups->n_windows, groups->n_seqs, e->cus); /* exact: the batch runs once */
    hipStream_t st;
    if ((rc = hold_sw(e, p.total, hip_stream, &st)) != CW_OK) return rc;
    uint8_t* base = (uint8_t*)e->scratch;
    StrandArgs a;
    a.b = dev_batch(groups);
    a.n_seqs = groups->n_seqs; a.strand = out->strand; a.hits = out->hits; a.k = out->k ? out->k : CW_STRAND_K;
    a.ctr = (uint32_t*)(base + p.ctr); a.unit_off = (uint32_t*)(base + p.unit_off);
    if ((rc = run_begin(e, st, true)) != CW_OK) return rc;
    CW_HIP(hipMemsetAsync(a.ctr, 0, (size_t)CW_STR_CTR_WORDS * 4, st));
    stage(e, st, "strand_order", [&] { cw_strand_units_kernel<<<1, 1024, 0, st>>>(a); });
    stage(e, st, "strand", [&] { cw_strand_kernel<0><<<p.wgs, CW_STR_THREADS, 0, st>>>(a); });
    stage(e, st, "strand_wide", [&] { cw_strand_kernel<1><<<p.wgs_wide, CW_STR_THREADS_WIDE, kLdsStrandWide, st>>>(a); });
    return run_end(e, st);
}

int validate_seed(const cw_engine* e, const cw_batch* groups, const cw_seeds* out) {
    if (!e || !groups || !out || !out->rows) return CW_E_INVALID;
    if (out->k != 0u && (out->k < CW_STRAND_KMIN || out->k > CW_STRAND_KMAX)) return CW_E_INVALID;
    return validate_groups(e, groups, out->rows);
}

/* the body of cw_seed_run_device; the caller holds e->mu.  Stages: strand_order (the strand run's units kernel as it is: it reads the batch, unit_off and ctr),
   seed (references of up to CW_ST_RMAX bases), seed_wide (beyond). */
int run_seed_locked(cw_engine* e, const cw_batch* groups, const cw_seeds* out, void* hip_stream) {
    int rc = validate_seed(e, groups, out);
    if (rc || groups->n_seqs == 0) return rc;
    const StrandPlan p = plan_seed(groups->n_windows, groups->n_seqs, e->cus); /* exact: the batch runs once */
    hipStream_t st;
    if ((rc = hold_sw(e, p.total, hip_stream, &st)) != CW_OK) return rc;
    uint8_t* base = (uint8_t*)e->scratch;
    SeedArgs a;
    a.b = dev_batch(groups);
    a.n_seqs = groups->n_seqs; a.rows = out->rows; a.strand = out->strand; a.k = out->k ? out->k : CW_STRAND_K;
    a.ctr = (uint32_t*)(base + p.ctr); a.unit_off = (uint32_t*)(base + p.unit_off);
    StrandArgs units; /* what cw_strand_units_kernel reads of it: the batch, unit_off and ctr */
    units.b = a.b; units.n_seqs = a.n_seqs; units.strand = nullptr; units.hits = nullptr; units.k = a.k;
    units.ctr = a.ctr; units.unit_off = (uint32_t*)(base + p.unit_off);
    if ((rc = run_begin(e, st, true)) != CW_OK) return rc;
    CW_HIP(hipMemsetAsync(a.ctr, 0, (size_t)CW_STR_CTR_WORDS * 4, st));
    stage(e, st, "strand_order", [&] { cw_strand_units_kernel<<<1, 1024, 0, st>>>(units); });
    stage(e, st, "seed", [&] { cw_seed_kernel<0><<<p.wgs, CW_STR_THREADS, 0, st>>>(a); });
    stage(e, st, "seed_wide", [&] { cw_seed_kernel<1><<<p.wgs_wide, CW_SEED_THREADS_WIDE, kLdsSeedWide, st>>>(a); });
    return run_end(e, st);
}

/* the body of cw_revcomp_device.  One stage: revcomp.  No scratch: what the engine's scratch holds stays what it was. */
int run_revcomp_locked(cw_engine* e, const cw_batch* groups, const uint8_t* strand, uint32_t* bases_out, void* hip_stream) {
    int rc = validate_revcomp(e, groups, bases_out);
    if (rc || groups->n_seqs == 0) return rc;
    CW_HIP(hipSetDevice(e->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : e->stream;
    RevcompArgs a;
    a.n_seqs = groups->n_seqs; a.seq_len = groups->seq_len; a.seq_word_off = groups->seq_word_off; a.bases = groups->bases; a.strand = strand; a.out = bases_out;
    const uint32_t per = 256u / CW_RC_LANES; /* sequences a work-group and round */
    const uint32_t wgs = (uint32_t)std::max<uint64_t>(1u, std::min<uint64_t>(((uint64_t)groups->n_seqs + per - 1u) / per, (uint64_t)e->cus * 32u));
    if ((rc = run_begin(e, st, false)) != CW_OK) return rc;
    stage(e, st, "revcomp", [&] { cw_revcomp_kernel<<<wgs, 256, 0, st>>>(a); });
    return run_end(e, st);
}

/* the body of cw_seed_spans_device; the caller holds e->mu.  One stage: seed_spans.  No scratch, as the reverse complement. */
int run_seed_spans_locked(cw_engine* e, const cw_batch* groups, const int32_t* seed_rows, uint32_t min_hits, uint32_t pad, uint32_t pad_shift, uint32_t* ref_lo, uint32_t* ref_hi,
                          void* hip_stream) {
    if (!e || !groups || pad_shift > 31u) return CW_E_INVALID;
    int rc = validate_groups(e, groups, seed_rows);
    if (rc || groups->n_seqs == 0) return rc;
    if (!ref_lo || !ref_hi) return CW_E_INVALID;
    CW_HIP(hipSetDevice(e->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : e->stream;
    SeedSpanArgs a;
    a.b = dev_batch(groups);
    a.n_seqs = groups->n_seqs; a.rows = seed_rows; a.min_hits = min_hits; a.pad = pad; a.pad_shift = pad_shift; a.ref_lo = ref_lo; a.ref_hi = ref_hi;
    if ((rc = run_begin(e, st, false)) != CW_OK) return rc;
    stage(e, st, "seed_spans", [&] { cw_seed_spans_kernel<<<(a.n_seqs + 255u) / 256u, 256, 0, st>>>(a); });
    return run_end(e, st);
}

/* ---- reads placed through an index of the whole reference: cw_locate_* ---------------------------------------------------------------------------------------- */

int validate_locate_ref(const cw_engine* e, const cw_locate_ref* ref) {
    if (!e || !ref || !ref->table || (ref->len > 0 && !ref->bases) || ref->len > CW_LOCATE_RMAX) return CW_E_INVALID;
    if (ref->k != 0u && (ref->k < CW_STRAND_KMIN || ref->k > CW_STRAND_KMAX)) return CW_E_INVALID;
    return CW_OK;
}

int validate_locate(const cw_engine* e, const cw_locate_ref* ref, const cw_batch* reads, const cw_seeds* out) {
    if (int rc = validate_locate_ref(e, ref)) return rc;
    if (!reads || !out || !out->rows) return CW_E_INVALID;
    if (out->k != 0u && out->k != (ref->k ? ref->k : CW_LOCATE_K)) return CW_E_INVALID;
    if (reads->n_seqs != 0 && (!reads->seq_len || !reads->seq_word_off || !reads->bases)) return CW_E_INVALID;
    return CW_OK;
}

LocateRefArgs locate_ref_args(const cw_locate_ref* ref) {
    LocateRefArgs r;
    r.ref = ref->bases; r.n = (uint32_t)ref->len; r.table = ref->table; r.bits = cw_loc_table_bits(ref->len); r.k = ref->k ? ref->k : CW_LOCATE_K;
    return r;
}

/* the body of cw_locate_build_device; the caller holds e->mu.  One stage: locate_build, the clear and the inserts.  No scratch, as the reverse complement. */
int run_locate_build_locked(cw_engine* e, const cw_locate_ref* ref, void* hip_stream) {
    int rc = validate_locate_ref(e, ref);
    if (rc) return rc;
    CW_HIP(hipSetDevice(e->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : e->stream;
    const LocateRefArgs r = locate_ref_args(ref);
    const uint64_t positions = r.n >= r.k ? (uint64_t)r.n - r.k + 1u : 0u;
    const uint32_t wgs = (uint32_t)std::max<uint64_t>(1u, std::min<uint64_t>((positions + 255u) / 256u, (uint64_t)e->cus * 32u));
    if ((rc = run_begin(e, st, false)) != CW_OK) return rc;
    hipError_t cleared = hipSuccess;
    stage(e, st, "locate_build", [&] {
        cleared = hipMemsetAsync(r.table, 0xFF, ((size_t)1 << r.bits) * 4, st); /* CW_STR_EMPTY in every slot */
        cw_locate_build_kernel<<<wgs, 256, 0, st>>>(r);
    });
    CW_HIP(cleared);
    return run_end(e, st);
}

/* the body of cw_locate_run_device; the caller holds e->mu.  Stages: locate (every read, the votes in LDS), locate_dense (the reads that route abandoned). */
int run_locate_locked(cw_engine* e, const cw_locate_ref* ref, const cw_batch* reads, const cw_seeds* out, void* hip_stream) {
    int rc = validate_locate(e, ref, reads, out);
    if (rc || reads->n_seqs == 0) return rc;
    const LocatePlan p = plan_locate(reads->n_seqs, e->cus); /* exact: the batch runs once */
    hipStream_t st;
    if ((rc = hold_sw(e, p.total, hip_stream, &st)) != CW_OK) return rc;
    if (!e->locate_routes) CW_HIP(hipMalloc((void**)&e->locate_routes, 8));
    uint8_t* base = (uint8_t*)e->scratch;
    LocateArgs a;
    a.r = locate_ref_args(ref);
    a.n_seqs = reads->n_seqs; a.seq_len = reads->seq_len; a.seq_word_off = reads->seq_word_off; a.bases = reads->bases;
    a.rows = out->rows; a.strand = out->strand;
    a.ctr = (uint32_t*)(base + p.ctr); a.redo = (uint32_t*)(base + p.redo); a.dense = (uint32_t*)(base + p.dense); a.routes = e->locate_routes;
    if ((rc = run_begin(e, st, true)) != CW_OK) return rc;
    CW_HIP(hipMemsetAsync(a.ctr, 0, (size_t)CW_LOC_CTR_WORDS * 4, st));
    stage(e, st, "locate", [&] { cw_locate_kernel<0><<<p.wgs, CW_LOC_THREADS, 0, st>>>(a); });
    stage(e, st, "locate_dense", [&] { cw_locate_kernel<1><<<p.wgs_dense, CW_LOC_THREADS, 0, st>>>(a); });
    return run_end(e, st);
}

/* ---- the reads of a set that overlap each other: cw_overlap_* -------------------------------------------------------------------------------------------------- */

int validate_overlap_reads(const cw_engine* e, const cw_batch* reads, const cw_overlap_params* prm) {
    if (!e || !reads || !prm) return CW_E_INVALID;
    if (prm->k != 0u && (prm->k < CW_STRAND_KMIN || prm->k > CW_STRAND_KMAX)) return CW_E_INVALID;
    if (prm->sample > CW_OVL_SAMPLE_MAX || prm->max_occ > CW_OVL_MAX_OCC_MAX) return CW_E_INVALID;
    if (reads->n_seqs > CW_OVL_READS_MAX) return CW_E_INVALID;
    if (reads->n_seqs != 0 && (!reads->seq_len || !reads->seq_word_off || !reads->bases)) return CW_E_INVALID;
    return CW_OK;
}

int validate_overlap_index(const cw_engine* e, const cw_batch* reads, const cw_overlap_index* index) {
    if (!index) return CW_E_INVALID;
    if (int rc = validate_overlap_reads(e, reads, &index->prm)) return rc;
    if (!index->mem || ((uintptr_t)index->mem & 7u) || index->n_entries > 0xFFFFFFFFull || index->prm.min_hits < 1u) return CW_E_INVALID;
    return CW_OK;
}

OvlIndexArgs overlap_index_args(const cw_batch* reads, const cw_overlap_params* prm, uint32_t* mem, uint64_t n_entries) {
    OvlIndexArgs x;
    memset(&x, 0, sizeof(x));
    x.bits = cw_ovl_table_bits(n_entries);
    const size_t slots = (size_t)1 << x.bits;
    x.hdr = mem;
    if (mem) { x.keys = mem + CW_OVL_HDR; x.cnt = x.keys + slots; x.off = x.cnt + slots; x.post = (unsigned long long*)(x.off + slots); x.counted = (unsigned long long*)(mem + 2); }
    x.n_entries = n_entries;
    x.k = prm->k ? prm->k : CW_OVL_K; x.sample = prm->sample; x.max_occ = prm->max_occ ? prm->max_occ : CW_OVL_MAX_OCC; x.min_hits = prm->min_hits;
    x.n_reads = reads->n_seqs; x.seq_len = reads->seq_len; x.seq_word_off = reads->seq_word_off; x.bases = reads->bases;
    return x;
}

uint32_t overlap_read_wgs(const cw_engine* e, uint32_t n_reads) { return (uint32_t)std::max<uint64_t>(1u, std::min<uint64_t>(n_reads, (uint64_t)e->cus * 32u)); }

/* the body of cw_overlap_count_device; the caller holds e->mu.  One stage, ovl_count, into the plan's counters; the one synchronisation reads them. */
int run_overlap_count_locked(cw_engine* e, const cw_batch* reads, const cw_overlap_params* prm, uint64_t* n_entries, void* hip_stream) {
    int rc = validate_overlap_reads(e, reads, prm);
    if (rc || !n_entries) return rc ? rc : CW_E_INVALID;
    *n_entries = 0;
    if (reads->n_seqs == 0) return CW_OK;
    const OverlapPlan p = plan_overlap(0, e->cus);
    hipStream_t st;
    if ((rc = hold_sw(e, p.total, hip_stream, &st)) != CW_OK) return rc;
    OvlIndexArgs x = overlap_index_args(reads, prm, nullptr, 0);
    x.counted = (unsigned long long*)((uint8_t*)e->scratch + p.ctr);
    if ((rc = run_begin(e, st, true)) != CW_OK) return rc;
    CW_HIP(hipMemsetAsync(x.counted, 0, (size_t)CW_OVL_CTR_WORDS * 4, st));
    stage(e, st, "ovl_count", [&] { cw_overlap_index_kernel<0><<<overlap_read_wgs(e, x.n_reads), 256, 0, st>>>(x); });
    if ((rc = run_end(e, st)) != CW_OK) return rc;
    unsigned long long got = 0;
    CW_HIP(hipMemcpyAsync(&got, x.counted, 8, hipMemcpyDeviceToHost, st));
    CW_HIP(hipStreamSynchronize(st));
    *n_entries = got;
    return CW_OK;
}

/* the body of cw_overlap_build_device; the caller holds e->mu.  No scratch: everything lives in the caller's memory. */
int run_overlap_build_locked(cw_engine* e, const cw_batch* reads, const cw_overlap_index* index, void* hip_stream) {
    int rc = validate_overlap_index(e, reads, index);
    if (rc) return rc;
    CW_HIP(hipSetDevice(e->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : e->stream;
    const OvlIndexArgs x = overlap_index_args(reads, &index->prm, index->mem, index->n_entries);
    const size_t slots = (size_t)1 << x.bits;
    const uint32_t wgs = overlap_read_wgs(e, x.n_reads), wgs_slots = (uint32_t)std::min<uint64_t>(slots / 256u, (uint64_t)e->cus * 32u);
    if ((rc = run_begin(e, st, false)) != CW_OK) return rc;
    hipError_t c0 = hipSuccess, c1 = hipSuccess, c2 = hipSuccess;
    stage(e, st, "ovl_build_count", [&] {
        c0 = hipMemsetAsync(x.hdr, 0, (size_t)CW_OVL_HDR * 4, st);
        c1 = hipMemsetAsync(x.keys, 0xFF, slots * 4, st); /* CW_STR_EMPTY in every slot */
        c2 = hipMemsetAsync(x.cnt, 0, slots * 8, st);     /* the counts and the offsets */
        cw_overlap_index_kernel<0><<<wgs, 256, 0, st>>>(x);
    });
    stage(e, st, "ovl_build_insert", [&] { cw_overlap_index_kernel<1><<<wgs, 256, 0, st>>>(x); });
    stage(e, st, "ovl_build_assign", [&] { cw_overlap_assign_kernel<<<wgs_slots, 256, 0, st>>>(x); });
    stage(e, st, "ovl_build_fill", [&] { cw_overlap_index_kernel<3><<<wgs, 256, 0, st>>>(x); cw_overlap_seal_kernel<<<1, 64, 0, st>>>(x); });
    CW_HIP(c0); CW_HIP(c1); CW_HIP(c2);
    return run_end(e, st);
}

int validate_overlap_run(const cw_engine* e, const cw_overlap_index* index, const cw_batch* reads, uint32_t first, uint32_t n_queries, const cw_overlaps* out) {
    if (int rc = validate_overlap_index(e, reads, index)) return rc;
    if (!out || (uint64_t)first + n_queries > reads->n_seqs) return CW_E_INVALID;
    if (n_queries != 0 && (!out->rows || !out->row_off || !out->n_rows || !out->status)) return CW_E_INVALID;
    return CW_OK;
}

/* the body of cw_overlap_run_device; the caller holds e->mu.  Stages: ovl (every query, the tables in LDS), ovl_dense (the queries that route abandoned). */
int run_overlap_locked(cw_engine* e, const cw_overlap_index* index, const cw_batch* reads, uint32_t first, uint32_t n_queries, const cw_overlaps* out, void* hip_stream) {
    int rc = validate_overlap_run(e, index, reads, first, n_queries, out);
    if (rc || n_queries == 0) return rc;
    const OverlapPlan p = plan_overlap(n_queries, e->cus); /* exact: the queries run once */
    hipStream_t st;
    if ((rc = hold_sw(e, p.total, hip_stream, &st)) != CW_OK) return rc;
    if (!e->ovl_routes) CW_HIP(hipMalloc((void**)&e->ovl_routes, 8));
    uint8_t* base = (uint8_t*)e->scratch;
    OvlArgs a;
    a.x = overlap_index_args(reads, &index->prm, index->mem, index->n_entries);
    a.first = first; a.n_queries = n_queries;
    a.rows = out->rows; a.row_off = out->row_off; a.n_rows = out->n_rows; a.status = out->status;
    a.ctr = (uint32_t*)(base + p.ctr); a.redo = (uint32_t*)(base + p.redo); a.dense = (uint32_t*)(base + p.dense); a.routes = e->ovl_routes;
    if ((rc = run_begin(e, st, true)) != CW_OK) return rc;
    CW_HIP(hipMemsetAsync(a.ctr, 0, (size_t)CW_OVL_CTR_WORDS * 4, st));
    stage(e, st, "ovl", [&] { cw_overlap_kernel<0><<<p.wgs, CW_OVL_THREADS, 0, st>>>(a); });
    stage(e, st, "ovl_dense", [&] { cw_overlap_kernel<1><<<p.wgs_dense, CW_OVL_THREADS, 0, st>>>(a); });
    return run_end(e, st);
}

/* the body of cw_overlap_to_pile_device; the caller holds e->mu.  No scratch. */
int run_overlap_pile_locked(cw_engine* e, const cw_overlaps* rows, uint32_t n_queries, uint32_t max_support, cw_overlap* pile, const uint64_t* pile_off, uint32_t* pile_n, void* hip_stream) {
    if (!e || !rows) return CW_E_INVALID;
    if (n_queries == 0) return CW_OK;
    if (!rows->rows || !rows->row_off || !rows->n_rows || !rows->status || !pile || !pile_off || !pile_n) return CW_E_INVALID;
    CW_HIP(hipSetDevice(e->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : e->stream;
    OvlPileArgs a;
    a.rows = rows->rows; a.row_off = rows->row_off; a.n_rows = rows->n_rows; a.status = rows->status;
    a.n_queries = n_queries; a.max_support = max_support; a.pile = pile; a.pile_off = pile_off; a.pile_n = pile_n;
    int rc;
    if ((rc = run_begin(e, st, false)) != CW_OK) return rc;
    stage(e, st, "ovl_pile", [&] { cw_overlap_to_pile_kernel<<<(uint32_t)std::min<uint64_t>(((uint64_t)n_queries + 255u) / 256u, (uint64_t)e->cus * 8u), 256, 0, st>>>(a); });
    return run_end(e, st);
}

} // namespace

extern "C" {

const char* cw_version(void) { return "consent_amd 0.1 (gfx950, HIP)"; }

const char* cw_strerror(int s) {
    switch (s) {
    case CW_OK: return "ok";
    case CW_E_INVALID: return "invalid argument or malformed batch";
    case CW_E_NO_DEVICE: return "no HIP device or HIP runtime error";
    case CW_E_NOMEM: return "out of memory";
    case CW_E_CAPACITY: return "at least one window exceeded a capacity (see win_status)";
    case CW_E_INTERNAL: return "internal error";
    default: return "unknown status";
    }
}

int cw_create(const cw_params* params, int device, cw_engine** out) {
    if (!out) return CW_E_INVALID;
    *out = nullptr;
    int rc = check_params(params);
    if (rc) return rc;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) return CW_E_NO_DEVICE;
    cw_engine* e = new (std::nothrow) cw_engine();
    if (!e) return CW_E_NOMEM;
    e->prm = *params;
    e->device = device;
    if (hipSetDevice(device) != hipSuccess || hipGetDeviceProperties(&e->prop, device) != hipSuccess ||
        hipStreamCreate(&e->stream) != hipSuccess) {
        delete e;
        return CW_E_NO_DEVICE;
    }
    e->cus = e->prop.multiProcessorCount > 0 ? e->prop.multiProcessorCount : 256;
    bool ok = hipEventCreate(&e->ev_fork) == hipSuccess && hipEventCreate(&e->ev_begin) == hipSuccess && hipEventCreate(&e->ev_end) == hipSuccess &&
              hipEventCreateWithFlags(&e->ev_join_s, hipEventDisableTiming) == hipSuccess;
    ok = ok && hipHostMalloc((void**)&e->host_fb, sizeof(cw_host_fb), hipHostMallocDefault) == hipSuccess;
    if (ok) memset(e->host_fb, 0, sizeof(cw_host_fb));
    for (int i = 0; i < 3 && ok; ++i) ok = hipStreamCreateWithFlags(&e->side[i], hipStreamNonBlocking) == hipSuccess && hipEventCreateWithFlags(&e->ev_join[i], hipEventDisableTiming) == hipSuccess;
    ok = ok && hipStreamCreateWithFlags(&e->stagger, hipStreamNonBlocking) == hipSuccess; /* (cw_internal.h: created here, after the side streams, for its place in the order) */
    for (int i = 0; i < CW_MAX_STAGES && ok; ++i) ok = hipEventCreate(&e->ev0[i]) == hipSuccess && hipEventCreate(&e->ev1[i]) == hipSuccess;
    for (int i = 0; i < CW_SLOTS && ok; ++i)
        ok = hipEventCreateWithFlags(&e->slot[i].ev_in, hipEventDisableTiming) == hipSuccess && hipEventCreateWithFlags(&e->slot[i].ev_done, hipEventDisableTiming) == hipSuccess;
    if (!ok) { cw_destroy(e); return CW_E_NO_DEVICE; }
    /* kernel attributes are per device: set them here, once per engine (not behind a process-wide flag) */
    if (set_kernel_attributes(e->prop) != CW_OK) { cw_destroy(e); return CW_E_NO_DEVICE; }
    *out = e;
    return CW_OK;
}

void cw_destroy(cw_engine* e) {
    if (!e) return;
    (void)hipSetDevice(e->device);
    (void)hipDeviceSynchronize();
    if (e->scratch) (void)hipFree(e->scratch);
    for (int i = 0; i < CW_SLOTS; ++i) {
        cw_slot& s = e->slot[i];
        if (s.dev_in) (void)hipFree(s.dev_in);
        if (s.dev_out) (void)hipFree(s.dev_out);
        if (s.pin_out) (void)hipHostFree(s.pin_out);
        if (s.ev_in) (void)hipEventDestroy(s.ev_in);
        if (s.ev_done) (void)hipEventDestroy(s.ev_done);
    }
    if (e->xscratch) (void)hipFree(e->xscratch);
    if (e->poa_in) (void)hipFree(e->poa_in);
    if (e->poa_out) (void)hipFree(e->poa_out);
    if (e->step_clock) (void)hipFree(e->step_clock);
    if (e->stitch_scratch) (void)hipFree(e->stitch_scratch);
    if (e->emitted) (void)hipFree(e->emitted);
    if (e->locate_tab) (void)hipFree(e->locate_tab);
    if (e->locate_routes) (void)hipFree(e->locate_routes);
    if (e->ovl_index) (void)hipFree(e->ovl_index);
    if (e->ovl_routes) (void)hipFree(e->ovl_routes);
    if (e->host_fb) (void)hipHostFree(e->host_fb);
    for (int i = 0; i < CW_MAX_STAGES; ++i) { if (e->ev0[i]) (void)hipEventDestroy(e->ev0[i]); if (e->ev1[i]) (void)hipEventDestroy(e->ev1[i]); }
    for (int i = 0; i < 3; ++i) { if (e->ev_join[i]) (void)hipEventDestroy(e->ev_join[i]); if (e->side[i]) (void)hipStreamDestroy(e->side[i]); }
    if (e->stagger) (void)hipStreamDestroy(e->stagger);
    if (e->ev_fork) (void)hipEventDestroy(e->ev_fork);
    if (e->ev_join_s) (void)hipEventDestroy(e->ev_join_s);
    if (e->ev_begin) (void)hipEventDestroy(e->ev_begin);
    if (e->ev_end) (void)hipEventDestroy(e->ev_end);
    if (e->copy_in) (void)hipStreamDestroy(e->copy_in);
    if (e->copy_out) (void)hipStreamDestroy(e->copy_out);
    if (e->stream) (void)hipStreamDestroy(e->stream);
    delete e;
}

int cw_run_device(cw_engine* e, const cw_batch* batch, const cw_result* res, void* hip_stream) {
    return locked(e, [&] { return run_device_locked(e, batch, res, hip_stream); });
}

int cw_poa_run_device(cw_engine* e, const cw_batch* groups, const cw_result* res, void* hip_stream) {
    return locked(e, [&] { return poa_device_locked(e, groups, res, hip_stream); });
}

/* Host buffers in, host buffers out, synchronous: the batch and the slot offsets go up, cw_poa_run_device on the engine's stream, lengths, statuses and the
   slots come back, and every consensus is copied into the caller's slot -- its own bytes only.  The caller holds e->mu throughout: the two device buffers are
   the engine's.  Its checks and its upload are its own; the layout, the hold step and the lock are the other host forms'. */
static int poa_run_host(cw_engine* e, const cw_batch* b, const cw_result* r) {
    int rc = validate_poa(e, b, r);
    if (rc || b->n_windows == 0) return rc;
    const uint32_t G = b->n_windows, S = b->n_seqs;
    if (b->win_first_seq[0] != 0 || b->win_first_seq[G] != S) return CW_E_INVALID;
    for (uint32_t g = 0; g < G; ++g) if (b->win_first_seq[g + 1] < b->win_first_seq[g] || r->cons_off[g + 1] < r->cons_off[g]) return CW_E_INVALID;
    for (uint32_t s = 0; s < S; ++s)
        if (b->seq_word_off[s] + ((uint64_t)b->seq_len[s] + 15) / 16 > b->n_words || b->seq_len[s] > 65535u) return CW_E_INVALID;
    const uint64_t c0 = r->cons_off[0], cons_bytes = r->cons_off[G] - c0;
    Layout in, out;
    const size_t i_wfs = in.put((size_t)(G + 1) * 4), i_len = in.put((size_t)S * 4), i_off = in.put((size_t)S * 8), i_bases = in.put((size_t)(b->n_words + 1) * 4),
                 i_coff = in.put((size_t)(G + 1) * 8);
    const size_t o_cons = out.put(cons_bytes), o_clen = out.put((size_t)G * 4), o_stat = out.put(G);
    std::vector<uint8_t> back;
    std::vector<uint64_t> coff; /* the slots' offsets in the device copy, which begins at the first slot */
    try { back.resize(out.bytes); coff.resize((size_t)G + 1); } catch (...) { return CW_E_NOMEM; }
    for (uint32_t g = 0; g <= G; ++g) coff[g] = r->cons_off[g] - c0;
    if ((rc = hold_io(e, in.bytes, out.bytes)) != CW_OK) return rc;
    uint8_t *din = (uint8_t*)e->poa_in, *dout = (uint8_t*)e->poa_out;
    hipStream_t st = e->stream;
    CW_HIP(hipMemcpyAsync(din + i_wfs, b->win_first_seq, (size_t)(G + 1) * 4, hipMemcpyHostToDevice, st));
    if (S) CW_HIP(hipMemcpyAsync(din + i_len, b->seq_len, (size_t)S * 4, hipMemcpyHostToDevice, st));
    if (S) CW_HIP(hipMemcpyAsync(din + i_off, b->seq_word_off, (size_t)S * 8, hipMemcpyHostToDevice, st));
    if (b->n_words) CW_HIP(hipMemcpyAsync(din + i_bases, b->bases, (size_t)b->n_words * 4, hipMemcpyHostToDevice, st));
    CW_HIP(hipMemsetAsync(din + i_bases + (size_t)b->n_words * 4, 0, 4, st));
    CW_HIP(hipMemcpyAsync(din + i_coff, coff.data(), (size_t)(G + 1) * 8, hipMemcpyHostToDevice, st));
    cw_batch db = *b;
    db.win_first_seq = (const uint32_t*)(din + i_wfs); db.seq_len = (const uint32_t*)(din + i_len);
    db.seq_word_off = (const uint64_t*)(din + i_off); db.bases = (const uint32_t*)(din + i_bases);
    cw_result dr;
    dr.cons = (char*)(dout + o_cons);
    dr.cons_off = (const uint64_t*)(din + i_coff); dr.cons_len = (uint32_t*)(dout + o_clen); dr.win_status = dout + o_stat;
    dr.solid = nullptr; dr.solid_off = nullptr; dr.solid_len = nullptr;
    if ((rc = poa_device_locked(e, &db, &dr, st)) != CW_OK) return rc;
    CW_HIP(hipMemcpyAsync(back.data(), dout, out.bytes, hipMemcpyDeviceToHost, st));
    CW_HIP(hipStreamSynchronize(st));
    const uint32_t* clen = (const uint32_t*)(back.data() + o_clen);
    for (uint32_t g = 0; g < G; ++g) {
        const bool ok = back[o_stat + g] != CW_WIN_OVERFLOW;
        if (!ok) rc = CW_E_CAPACITY;
        r->win_status[g] = back[o_stat + g];
        r->cons_len[g] = ok ? clen[g] : 0u;
        if (ok && clen[g]) memcpy(r->cons + r->cons_off[g], back.data() + o_cons + coff[g], clen[g]);
    }
    return rc;
}

int cw_poa_run(cw_engine* e, const cw_batch* b, const cw_result* r) {
    return locked(e, [&] { return poa_run_host(e, b, r); });
}

int cw_sw_run_device(cw_engine* e, const cw_batch* groups, int32_t* rows, uint32_t flags, void* hip_stream) {
    return locked(e, [&] { return run_sw_locked(e, groups, rows, flags, hip_stream); });
}

int cw_sw_span_run_device(cw_engine* e, const cw_batch* groups, int32_t* rows, const cw_sw_spans* spans, uint32_t flags, void* hip_stream) {
    return spans ? locked(e, [&] { return run_sw_locked(e, groups, rows, flags, hip_stream, spans); }) : CW_E_INVALID;
}

/* The host forms (HostTrip, above): each states its validation, its slot offsets, its outputs, what else goes up, its device form and what of the caller's
   bytes it writes on the way back.  One body for cw_sw_run and cw_sw_span_run, as for the three pairs below: a span run's two arrays go up with the batch.
   This one: the rows come back. */
static int sw_run_host(cw_engine* e, const cw_batch* b, int32_t* rows, uint32_t flags, const cw_sw_spans* spans) {
    if (!e) return CW_E_INVALID;
    HostTrip t(e, b, spans);
    int rc = validate_sw(e, b, rows, flags);
    if (!rc) rc = validate_spans(spans, b->n_seqs);
    if (rc || b->n_seqs == 0) return rc;
    if ((rc = t.check_groups(nullptr)) != CW_OK) return rc;
    const uint32_t S = b->n_seqs;
    const size_t row_bytes = (size_t)S * CW_SW_ROW * 4, o_rows = t.out.put(row_bytes);
    if ((rc = t.upload_groups()) != CW_OK) return rc;
    if ((rc = run_sw_locked(e, &t.db, t.at<int32_t>(o_rows), flags, t.st, t.dev_spans())) != CW_OK) return rc;
    CW_HIP(t.down(rows, o_rows, row_bytes));
    CW_HIP(t.sync());
    return sw_rows_rc(rows, S);
}

int cw_sw_run(cw_engine* e, const cw_batch* b, int32_t* rows, uint32_t flags) { return sw_run_host(e, b, rows, flags, nullptr); }
int cw_sw_span_run(cw_engine* e, const cw_batch* b, int32_t* rows, const cw_sw_spans* spans, uint32_t flags) { return spans ? sw_run_host(e, b, rows, flags, spans) : CW_E_INVALID; }

int cw_sw_path_run_device(cw_engine* e, const cw_batch* groups, int32_t* rows, const cw_sw_paths* paths, uint32_t flags, void* hip_stream) {
    return locked(e, [&] { return run_sw_path_locked(e, groups, rows, paths, flags, hip_stream); });
}

int cw_sw_path_span_run_device(cw_engine* e, const cw_batch* groups, int32_t* rows, const cw_sw_paths* paths, const cw_sw_spans* spans, uint32_t flags, void* hip_stream) {
    return spans ? locked(e, [&] { return run_sw_path_locked(e, groups, rows, paths, flags, hip_stream, spans); }) : CW_E_INVALID;
}

/* Rows and op counts come back -- and of the ops only what was written: a slot's words beyond its path, and every slot without one, stay the caller's. */
static int sw_path_run_host(cw_engine* e, const cw_batch* b, int32_t* rows, const cw_sw_paths* paths, uint32_t flags, const cw_sw_spans* spans) {
    if (!e) return CW_E_INVALID;
    HostTrip t(e, b, spans);
    int rc = validate_sw_path(e, b, rows, paths, flags);
    if (!rc) rc = validate_spans(spans, b->n_seqs);
    if (rc || b->n_seqs == 0) return rc;
    if ((rc = t.check_groups(paths->ops_off)) != CW_OK) return rc;
    const uint32_t S = b->n_seqs;
    const std::vector<uint64_t>& poff = t.slot;
    const size_t row_bytes = (size_t)S * CW_SW_ROW * 4, op_bytes = (size_t)poff[S] * 4;
    const size_t o_rows = t.out.put(row_bytes), o_nops = t.out.put((size_t)S * 4), o_ops = t.out.put(op_bytes);
    std::vector<uint32_t> back;
    try { back.resize((size_t)poff[S]); } catch (...) { return CW_E_NOMEM; }
    if ((rc = t.upload_groups()) != CW_OK) return rc;
    cw_sw_paths dp;
    dp.ops = t.at<uint32_t>(o_ops); dp.ops_off = t.d_slot; dp.n_ops = t.at<uint32_t>(o_nops);
    if ((rc = run_sw_path_locked(e, &t.db, t.at<int32_t>(o_rows), &dp, flags, t.st, t.dev_spans())) != CW_OK) return rc;
    CW_HIP(t.down(rows, o_rows, row_bytes));
    CW_HIP(t.down(paths->n_ops, o_nops, (size_t)S * 4));
    CW_HIP(t.down(back.data(), o_ops, op_bytes));
    CW_HIP(t.sync());
    for (uint32_t s = 0; s < S; ++s)
        if (rows[(size_t)s * CW_SW_ROW + CW_SW_STATUS] == CW_SW_ALIGNED && paths->n_ops[s] && paths->n_ops[s] <= poff[s + 1] - poff[s])
            memcpy(paths->ops + paths->ops_off[s], back.data() + poff[s], (size_t)paths->n_ops[s] * 4);
    return sw_rows_rc(rows, S);
}

int cw_sw_path_run(cw_engine* e, const cw_batch* b, int32_t* rows, const cw_sw_paths* paths, uint32_t flags) { return sw_path_run_host(e, b, rows, paths, flags, nullptr); }
int cw_sw_path_span_run(cw_engine* e, const cw_batch* b, int32_t* rows, const cw_sw_paths* paths, const cw_sw_spans* spans, uint32_t flags) {
    return spans ? sw_path_run_host(e, b, rows, paths, flags, spans) : CW_E_INVALID;
}

int cw_pileup_run_device(cw_engine* e, const cw_batch* groups, int32_t* rows, const cw_pileup* pile, uint32_t flags, void* hip_stream) {
    return locked(e, [&] { return run_pileup_locked(e, groups, rows, pile, flags, hip_stream); });
}

int cw_pileup_span_run_device(cw_engine* e, const cw_batch* groups, int32_t* rows, const cw_pileup* pile, const cw_sw_spans* spans, uint32_t flags, void* hip_stream) {
    return spans ? locked(e, [&] { return run_pileup_locked(e, groups, rows, pile, flags, hip_stream, spans); }) : CW_E_INVALID;
}

/* The caller's counts go up too, but only under CW_PILE_ACCUMULATE; the rows come back, and of the counts what a run owns: columns 0 .. ref_len - 1 of every
   reference whose slot holds them.  A slot's words beyond those, a slot that is too short and every query's slot stay the caller's. */
static int pileup_run_host(cw_engine* e, const cw_batch* b, int32_t* rows, const cw_pileup* pile, uint32_t flags, const cw_sw_spans* spans) {
    if (!e) return CW_E_INVALID;
    HostTrip t(e, b, spans);
    int rc = validate_pileup(e, b, rows, pile, flags);
    if (!rc) rc = validate_spans(spans, b->n_seqs);
    if (rc || b->n_seqs == 0) return rc;
    if ((rc = t.check_groups(pile->col_off)) != CW_OK) return rc;
    const uint32_t G = b->n_windows, S = b->n_seqs;
    const std::vector<uint64_t>& coff = t.slot;
    const size_t col_bytes = (size_t)CW_PILE_COL * 4, row_bytes = (size_t)S * CW_SW_ROW * 4, count_bytes = (size_t)coff[S] * col_bytes;
    const size_t o_rows = t.out.put(row_bytes), o_counts = t.out.put(count_bytes);
    std::vector<uint32_t> back;
    std::vector<std::pair<uint32_t, uint32_t>> owned; /* the references whose columns the run owns: (sequence, columns) */
    try {
        back.resize((size_t)coff[S] * CW_PILE_COL);
        for (uint32_t g = 0; g < G; ++g) {
            const uint32_t r = b->win_first_seq[g];
            if (r < b->win_first_seq[g + 1] && b->seq_len[r] && coff[r + 1] - coff[r] >= b->seq_len[r]) owned.emplace_back(r, b->seq_len[r]);
        }
    } catch (...) { return CW_E_NOMEM; }
    if ((rc = t.upload_groups()) != CW_OK) return rc;
    cw_pileup dp;
    dp.counts = t.at<uint32_t>(o_counts); dp.col_off = t.d_slot;
    if (flags & CW_PILE_ACCUMULATE) /* every slot in one copy; the run reads and writes the owned columns only */
        CW_HIP(t.up(o_counts, pile->counts + pile->col_off[0] * CW_PILE_COL, count_bytes));
    if ((rc = run_pileup_locked(e, &t.db, t.at<int32_t>(o_rows), &dp, flags, t.st, t.dev_spans())) != CW_OK) return rc;
    CW_HIP(t.down(rows, o_rows, row_bytes));
    CW_HIP(t.down(back.data(), o_counts, count_bytes));
    CW_HIP(t.sync());
    for (const auto& rn : owned)
        memcpy(pile->counts + pile->col_off[rn.first] * CW_PILE_COL, back.data() + coff[rn.first] * CW_PILE_COL, (size_t)rn.second * col_bytes);
    return sw_rows_rc(rows, S);
}

int cw_pileup_run(cw_engine* e, const cw_batch* b, int32_t* rows, const cw_pileup* pile, uint32_t flags) { return pileup_run_host(e, b, rows, pile, flags, nullptr); }
int cw_pileup_span_run(cw_engine* e, const cw_batch* b, int32_t* rows, const cw_pileup* pile, const cw_sw_spans* spans, uint32_t flags) {
    return spans ? pileup_run_host(e, b, rows, pile, flags, spans) : CW_E_INVALID;
}

int cw_sw_cut_run_device(cw_engine* e, const cw_batch* groups, int32_t* rows, const cw_sw_cuts* cuts, void* hip_stream) {
    return locked(e, [&] { return run_sw_cut_locked(e, groups, rows, cuts, hip_stream); });
}

int cw_sw_cut_span_run_device(cw_engine* e, const cw_batch* groups, int32_t* rows, const cw_sw_cuts* cuts, const cw_sw_spans* spans, void* hip_stream) {
    return spans ? locked(e, [&] { return run_sw_cut_locked(e, groups, rows, cuts, hip_stream, spans); }) : CW_E_INVALID;
}

/* The rows come back, and of the slots what a run owns: the T + 1 words of every query whose slot holds them.  A slot's words beyond those, a slot that is too
   short and every reference's slot stay the caller's. */
static int sw_cut_run_host(cw_engine* e, const cw_batch* b, int32_t* rows, const cw_sw_cuts* cuts, const cw_sw_spans* spans) {
    if (!e) return CW_E_INVALID;
    HostTrip t(e, b, spans);
    int rc = validate_sw_cut(e, b, rows, cuts);
    if (!rc) rc = validate_spans(spans, b->n_seqs);
    if (rc || b->n_seqs == 0) return rc;
    if ((rc = t.check_groups(cuts->cut_off)) != CW_OK) return rc;
    const uint32_t G = b->n_windows, S = b->n_seqs, W = cuts->window;
    const std::vector<uint64_t>& coff = t.slot;
    const size_t row_bytes = (size_t)S * CW_SW_ROW * 4, cut_bytes = (size_t)coff[S] * 4;
    const size_t o_rows = t.out.put(row_bytes), o_cuts = t.out.put(cut_bytes);
    std::vector<uint32_t> back;
    std::vector<std::pair<uint32_t, uint32_t>> owned; /* the queries whose words the run owns: (sequence, words) */
    try {
        back.resize((size_t)coff[S]);
        for (uint32_t g = 0; g < G; ++g) {
            const uint32_t r = b->win_first_seq[g], end = b->win_first_seq[g + 1];
            if (r >= end) continue;
            const uint32_t words = CW_SW_CUTS(b->seq_len[r], W);
            for (uint32_t s = r + 1; s < end; ++s) if (coff[s + 1] - coff[s] >= words) owned.emplace_back(s, words);
        }
    } catch (...) { return CW_E_NOMEM; }
    if ((rc = t.upload_groups()) != CW_OK) return rc;
    cw_sw_cuts dc;
    dc.cuts = t.at<uint32_t>(o_cuts); dc.cut_off = t.d_slot; dc.window = W;
    if ((rc = run_sw_cut_locked(e, &t.db, t.at<int32_t>(o_rows), &dc, t.st, t.dev_spans())) != CW_OK) return rc;
    CW_HIP(t.down(rows, o_rows, row_bytes));
    CW_HIP(t.down(back.data(), o_cuts, cut_bytes));
    CW_HIP(t.sync());
    for (const auto& sw : owned)
        if (rows[(size_t)sw.first * CW_SW_ROW + CW_SW_STATUS] != CW_SW_CUT_SLOT)
            memcpy(cuts->cuts + cuts->cut_off[sw.first], back.data() + coff[sw.first], (size_t)sw.second * 4);
    return sw_rows_rc(rows, S);
}

int cw_sw_cut_run(cw_engine* e, const cw_batch* b, int32_t* rows, const cw_sw_cuts* cuts) { return sw_cut_run_host(e, b, rows, cuts, nullptr); }
int cw_sw_cut_span_run(cw_engine* e, const cw_batch* b, int32_t* rows, const cw_sw_cuts* cuts, const cw_sw_spans* spans) { return spans ? sw_cut_run_host(e, b, rows, cuts, spans) : CW_E_INVALID; }

int cw_strand_run_device(cw_engine* e, const cw_batch* groups, const cw_strands* out, void* hip_stream) {
    return locked(e, [&] { return run_strand_locked(e, groups, out, hip_stream); });
}

/* The strand bytes and -- when asked for -- the hits come back. */
int cw_strand_run(cw_engine* e, const cw_batch* b, const cw_strands* out) {
    if (!e) return CW_E_INVALID;
    HostTrip t(e, b);
    int rc = validate_strand(e, b, out);
    if (rc || b->n_seqs == 0) return rc;
    if ((rc = t.check_groups(nullptr)) != CW_OK) return rc;
    const uint32_t S = b->n_seqs;
    const size_t o_strand = t.out.put(S), o_hits = t.out.put(out->hits ? (size_t)S * 8 : 0);
    if ((rc = t.upload_groups()) != CW_OK) return rc;
    cw_strands ds;
    ds.strand = t.at<uint8_t>(o_strand); ds.hits = out->hits ? t.at<uint32_t>(o_hits) : nullptr; ds.k = out->k;
    if ((rc = run_strand_locked(e, &t.db, &ds, t.st)) != CW_OK) return rc;
    CW_HIP(t.down(out->strand, o_strand, S));
    if (out->hits) CW_HIP(t.down(out->hits, o_hits, (size_t)S * 8));
    CW_HIP(t.sync());
    return CW_OK;
}

int cw_seed_run_device(cw_engine* e, const cw_batch* groups, const cw_seeds* out, void* hip_stream) {
    return locked(e, [&] { return run_seed_locked(e, groups, out, hip_stream); });
}

/* The rows and -- when asked for -- the strand bytes come back. */
int cw_seed_run(cw_engine* e, const cw_batch* b, const cw_seeds* out) {
    if (!e) return CW_E_INVALID;
    HostTrip t(e, b);
    int rc = validate_seed(e, b, out);
    if (rc || b->n_seqs == 0) return rc;
    if ((rc = t.check_groups(nullptr)) != CW_OK) return rc;
    const uint32_t S = b->n_seqs;
    const size_t row_bytes = (size_t)S * CW_SEED_ROW * 4, o_rows = t.out.put(row_bytes), o_strand = t.out.put(out->strand ? (size_t)S : 0);
    if ((rc = t.upload_groups()) != CW_OK) return rc;
    cw_seeds ds;
    ds.rows = t.at<int32_t>(o_rows); ds.strand = out->strand ? t.at<uint8_t>(o_strand) : nullptr; ds.k = out->k;
    if ((rc = run_seed_locked(e, &t.db, &ds, t.st)) != CW_OK) return rc;
    CW_HIP(t.down(out->rows, o_rows, row_bytes));
    if (out->strand) CW_HIP(t.down(out->strand, o_strand, S));
    CW_HIP(t.sync());
    return CW_OK;
}

int cw_seed_spans_device(cw_engine* e, const cw_batch* groups, const int32_t* seed_rows, uint32_t min_hits, uint32_t pad, uint32_t pad_shift, uint32_t* ref_lo, uint32_t* ref_hi,
                         void* hip_stream) {
    return locked(e, [&] { return run_seed_spans_locked(e, groups, seed_rows, min_hits, pad, pad_shift, ref_lo, ref_hi, hip_stream); });
}

/* The seed rows go up with the batch; the two arrays come back. */
int cw_seed_spans(cw_engine* e, const cw_batch* b, const int32_t* seed_rows, uint32_t min_hits, uint32_t pad, uint32_t pad_shift, uint32_t* ref_lo, uint32_t* ref_hi) {
    if (!e || !b || pad_shift > 31u) return CW_E_INVALID;
    HostTrip t(e, b);
    int rc = validate_groups(e, b, seed_rows);
    if (rc || b->n_seqs == 0) return rc;
    if (!ref_lo || !ref_hi) return CW_E_INVALID;
    if ((rc = t.check_groups(nullptr)) != CW_OK) return rc;
    const uint32_t S = b->n_seqs;
    const size_t row_bytes = (size_t)S * CW_SEED_ROW * 4, o_rows = t.out.put(row_bytes), o_lo = t.out.put((size_t)S * 4), o_hi = t.out.put((size_t)S * 4);
    if ((rc = t.upload_groups()) != CW_OK) return rc;
    CW_HIP(t.up(o_rows, seed_rows, row_bytes));
    if ((rc = run_seed_spans_locked(e, &t.db, t.at<int32_t>(o_rows), min_hits, pad, pad_shift, t.at<uint32_t>(o_lo), t.at<uint32_t>(o_hi), t.st)) != CW_OK) return rc;
    CW_HIP(t.down(ref_lo, o_lo, (size_t)S * 4));
    CW_HIP(t.down(ref_hi, o_hi, (size_t)S * 4));
    CW_HIP(t.sync());
    return CW_OK;
}

int cw_revcomp_device(cw_engine* e, const cw_batch* groups, const uint8_t* strand, uint32_t* bases_out, void* hip_stream) {
    return locked(e, [&] { return run_revcomp_locked(e, groups, strand, bases_out, hip_stream); });
}

/* The strand bytes go up with the batch; of the words that come back every sequence's own are copied to bases_out: a word that belongs to no sequence is not
   written on the host either. */
int cw_revcomp(cw_engine* e, const cw_batch* b, const uint8_t* strand, uint32_t* bases_out) {
    if (!e) return CW_E_INVALID;
    HostTrip t(e, b);
    int rc = validate_revcomp(e, b, bases_out);
    if (rc || b->n_seqs == 0) return rc;
    if ((rc = t.check_groups(nullptr)) != CW_OK) return rc;
    const uint32_t S = b->n_seqs;
    const size_t o_words = t.out.put((size_t)(b->n_words + 1) * 4), o_strand = t.out.put(S);
    std::vector<uint32_t> back;
    try { back.resize((size_t)b->n_words + 1); } catch (...) { return CW_E_NOMEM; }
    if ((rc = t.upload_groups()) != CW_OK) return rc;
    if (strand) CW_HIP(t.up(o_strand, strand, S));
    if ((rc = run_revcomp_locked(e, &t.db, strand ? t.at<uint8_t>(o_strand) : nullptr, t.at<uint32_t>(o_words), t.st)) != CW_OK) return rc;
    CW_HIP(t.down(back.data(), o_words, (size_t)b->n_words * 4));
    CW_HIP(t.sync());
    for (uint32_t s = 0; s < S; ++s) {
        const size_t nw = ((size_t)b->seq_len[s] + 15) / 16;
        if (nw) memcpy(bases_out + b->seq_word_off[s], back.data() + b->seq_word_off[s], nw * 4);
    }
    return CW_OK;
}

/* Debug/inspection (cw_private.h): what plan_strand would allocate and its grids (host arithmetic only). */
int cw_debug_strand_plan(uint32_t n_groups, uint32_t n_seqs, int cus, uint64_t* out5) {
    if (!out5 || cus < 1) return CW_E_INVALID;
    const StrandPlan p = plan_strand(n_groups, n_seqs, cus);
    const uint64_t v[5] = {p.total, (uint64_t)p.unit_off, (uint64_t)(p.total - p.unit_off), p.wgs, p.wgs_wide};
    for (int i = 0; i < 5; ++i) out5[i] = v[i];
    return CW_OK;
}

uint64_t cw_locate_table_words(uint64_t ref_len) { return ref_len > CW_LOCATE_RMAX ? 0u : (uint64_t)1 << cw_loc_table_bits(ref_len); }

int cw_locate_build_device(cw_engine* e, const cw_locate_ref* ref, void* hip_stream) {
    return locked(e, [&] { return run_locate_build_locked(e, ref, hip_stream); });
}

int cw_locate_run_device(cw_engine* e, const cw_locate_ref* ref, const cw_batch* reads, const cw_seeds* out, void* hip_stream) {
    return locked(e, [&] { return run_locate_locked(e, ref, reads, out, hip_stream); });
}

/* The reference goes up behind the reads, the index is built into the engine's own table, the rows and -- when asked for -- the strand bytes come back.  The
   reads travel as one group: their grouping is not read, so the caller's is not looked at. */
int cw_locate_run(cw_engine* e, const uint32_t* ref_bases, uint64_t ref_len, uint32_t k, const cw_batch* reads, const cw_seeds* out) {
    if (!e) return CW_E_INVALID;
    uint32_t dummy_table = 0; /* (validation asks for a table: the engine's is held below) */
    cw_locate_ref ref;
    ref.bases = ref_bases; ref.len = ref_len; ref.table = &dummy_table; ref.k = k;
    const uint32_t one_group[2] = {0u, reads ? reads->n_seqs : 0u};
    cw_batch one;
    memset(&one, 0, sizeof(one));
    if (reads) { one = *reads; one.n_windows = 1; one.win_first_seq = one_group; }
    HostTrip t(e, &one);
    int rc = validate_locate(e, &ref, reads, out);
    if (rc || reads->n_seqs == 0) return rc;
    if ((rc = t.check_groups(nullptr)) != CW_OK) return rc;
    const uint32_t S = reads->n_seqs;
    const size_t ref_bytes = (size_t)((ref_len + 15) / 16) * 4, table_bytes = (size_t)cw_locate_table_words(ref_len) * 4;
    const size_t row_bytes = (size_t)S * CW_SEED_ROW * 4, o_rows = t.out.put(row_bytes), o_strand = t.out.put(out->strand ? (size_t)S : 0), o_ref = t.out.put(ref_bytes + 4);
    CW_HIP(hipSetDevice(e->device));
    if ((rc = ensure(&e->locate_tab, &e->locate_tab_bytes, table_bytes)) != CW_OK) return rc;
    if ((rc = t.upload_groups()) != CW_OK) return rc;
    CW_HIP(t.up(o_ref, ref_bases, ref_bytes));
    ref.bases = t.at<uint32_t>(o_ref); ref.table = (uint32_t*)e->locate_tab;
    cw_seeds ds;
    ds.rows = t.at<int32_t>(o_rows); ds.strand = out->strand ? t.at<uint8_t>(o_strand) : nullptr; ds.k = out->k;
    if ((rc = run_locate_build_locked(e, &ref, t.st)) != CW_OK) return rc;
    if ((rc = run_locate_locked(e, &ref, &t.db, &ds, t.st)) != CW_OK) return rc;
    CW_HIP(t.down(out->rows, o_rows, row_bytes));
    if (out->strand) CW_HIP(t.down(out->strand, o_strand, S));
    CW_HIP(t.sync());
    return CW_OK;
}

/* Debug/inspection (cw_private.h): what plan_locate would allocate and its grids (host arithmetic only). */
int cw_debug_locate_plan(uint32_t n_seqs, int cus, uint64_t* out6) {
    if (!out6 || cus < 1) return CW_E_INVALID;
    const LocatePlan p = plan_locate(n_seqs, cus);
    const uint64_t v[6] = {p.total, (uint64_t)(p.redo - p.ctr), (uint64_t)(p.dense - p.redo), (uint64_t)(p.total - p.dense), p.wgs, p.wgs_dense};
    for (int i = 0; i < 6; ++i) out6[i] = v[i];
    return CW_OK;
}

/* Debug/inspection (cw_private.h): the two words the last locate run's dense launch wrote, once everything on the device has ended. */
int cw_debug_locate_routes(cw_engine* e, uint32_t* out2) {
    if (!e || !out2) return CW_E_INVALID;
    std::lock_guard<std::mutex> lk(e->mu);
    if (!e->locate_routes) return CW_E_INVALID;
    CW_HIP(hipSetDevice(e->device));
    CW_HIP(hipDeviceSynchronize());
    CW_HIP(hipMemcpy(out2, e->locate_routes, 8, hipMemcpyDeviceToHost));
    return CW_OK;
}

uint64_t cw_overlap_index_words(uint64_t n_entries) { return n_entries > 0xFFFFFFFFull ? 0u : cw_ovl_index_words(n_entries); }

int cw_overlap_count_device(cw_engine* e, const cw_batch* reads, const cw_overlap_params* prm, uint64_t* n_entries, void* hip_stream) {
    return locked(e, [&] { return run_overlap_count_locked(e, reads, prm, n_entries, hip_stream); });
}

int cw_overlap_build_device(cw_engine* e, const cw_batch* reads, const cw_overlap_index* index, void* hip_stream) {
    return locked(e, [&] { return run_overlap_build_locked(e, reads, index, hip_stream); });
}

int cw_overlap_run_device(cw_engine* e, const cw_overlap_index* index, const cw_batch* reads, uint32_t first_query, uint32_t n_queries, const cw_overlaps* out, void* hip_stream) {
    return locked(e, [&] { return run_overlap_locked(e, index, reads, first_query, n_queries, out, hip_stream); });
}

int cw_overlap_to_pile_device(cw_engine* e, const cw_overlaps* rows, uint32_t n_queries, uint32_t max_support, cw_overlap* pile, const uint64_t* pile_off, uint32_t* pile_n, void* hip_stream) {
    return locked(e, [&] { return run_overlap_pile_locked(e, rows, n_queries, max_support, pile, pile_off, pile_n, hip_stream); });
}

/* The reads go up as one group, are counted (the form's one extra wait), indexed in the engine's own memory and run, all of them; rows, counts and statuses
   come back.  The slots' offsets are rebased to the first, as every host form's. */
int cw_overlap_run(cw_engine* e, const cw_batch* reads, const cw_overlap_params* prm, const cw_overlaps* out) {
    if (!e) return CW_E_INVALID;
    const uint32_t one_group[2] = {0u, reads ? reads->n_seqs : 0u};
    cw_batch one;
    memset(&one, 0, sizeof(one));
    if (reads) { one = *reads; one.n_windows = 1; one.win_first_seq = one_group; }
    HostTrip t(e, &one);
    int rc = validate_overlap_reads(e, reads, prm);
    if (rc) return rc;
    if (prm->min_hits < 1u || !out) return CW_E_INVALID;
    const uint32_t S = reads->n_seqs;
    if (S == 0) return CW_OK;
    if (!out->rows || !out->row_off || !out->n_rows || !out->status) return CW_E_INVALID;
    if ((rc = t.check_groups(out->row_off)) != CW_OK) return rc;
    const size_t row_bytes = (size_t)t.slot[S] * CW_OVL_ROW * 4;
    const size_t o_rows = t.out.put(row_bytes), o_n = t.out.put((size_t)S * 4), o_status = t.out.put(S);
    if ((rc = t.upload_groups()) != CW_OK) return rc;
    uint64_t n_entries = 0;
    if ((rc = run_overlap_count_locked(e, &t.db, prm, &n_entries, t.st)) != CW_OK) return rc;
    if (n_entries > 0xFFFFFFFFull) return CW_E_CAPACITY;
    if ((rc = ensure(&e->ovl_index, &e->ovl_index_bytes, (size_t)cw_ovl_index_words(n_entries) * 4)) != CW_OK) return rc;
    cw_overlap_index index;
    index.mem = (uint32_t*)e->ovl_index; index.n_entries = n_entries; index.prm = *prm;
    cw_overlaps d;
    d.rows = t.at<int32_t>(o_rows); d.row_off = t.d_slot; d.n_rows = t.at<uint32_t>(o_n); d.status = t.at<uint8_t>(o_status);
    if ((rc = run_overlap_build_locked(e, &t.db, &index, t.st)) != CW_OK) return rc;
    if ((rc = run_overlap_locked(e, &index, &t.db, 0, S, &d, t.st)) != CW_OK) return rc;
    CW_HIP(t.down(out->rows + out->row_off[0] * CW_OVL_ROW, o_rows, row_bytes));
    CW_HIP(t.down(out->n_rows, o_n, (size_t)S * 4));
    CW_HIP(t.down(out->status, o_status, S));
    CW_HIP(t.sync());
    for (uint32_t s = 0; s < S; ++s) if (out->status[s] == CW_OVL_SLOT || out->status[s] == CW_OVL_DENSE) return CW_E_CAPACITY;
    return CW_OK;
}

/* Debug/inspection (cw_private.h): what plan_overlap would allocate and its grids (host arithmetic only). */
int cw_debug_overlap_plan(uint32_t n_queries, int cus, uint64_t* out6) {
    if (!out6 || cus < 1) return CW_E_INVALID;
    const OverlapPlan p = plan_overlap(n_queries, cus);
    const uint64_t v[6] = {p.total, (uint64_t)(p.redo - p.ctr), (uint64_t)(p.dense - p.redo), (uint64_t)(p.total - p.dense), p.wgs, p.wgs_dense};
    for (int i = 0; i < 6; ++i) out6[i] = v[i];
    return CW_OK;
}

/* Debug/inspection (cw_private.h): the two words the last overlap run's dense launch wrote, once everything on the device has ended. */
int cw_debug_overlap_routes(cw_engine* e, uint32_t* out2) {
    if (!e || !out2) return CW_E_INVALID;
    std::lock_guard<std::mutex> lk(e->mu);
    if (!e->ovl_routes) return CW_E_INVALID;
    CW_HIP(hipSetDevice(e->device));
    CW_HIP(hipDeviceSynchronize());
    CW_HIP(hipMemcpy(out2, e->ovl_routes, 8, hipMemcpyDeviceToHost));
    return CW_OK;
}

/* Debug/inspection (cw_private.h): the same for plan_seed. */
int cw_debug_seed_plan(uint32_t n_groups, uint32_t n_seqs, int cus, uint64_t* out5) {
    if (!out5 || cus < 1) return CW_E_INVALID;
    const StrandPlan p = plan_seed(n_groups, n_seqs, cus);
    const uint64_t v[5] = {p.total, (uint64_t)p.unit_off, (uint64_t)(p.total - p.unit_off), p.wgs, p.wgs_wide};
    for (int i = 0; i < 5; ++i) out5[i] = v[i];
    return CW_OK;
}

/* One work-group sizes the output groups of every input group, a wave per output group counts its members and words, one work-group scans; the totals come to
   the host (the one synchronisation), and when they fit the same waves fill.  The working arrays live in the engine's scratch allocation -- the cut run's
   scratch is dead by then -- sized for the most output groups the batch's words can hold: 16 n_words / W + a group's last window each. */
int cw_cut_groups_device(cw_engine* e, const cw_batch* groups, const int32_t* rows, const cw_sw_cuts* cuts, uint32_t* grp_first, uint32_t* win_first_seq,
                         uint32_t* seq_len, uint64_t* seq_word_off, uint32_t* bases, uint32_t group_cap, uint32_t seq_cap, uint64_t word_cap,
                         uint32_t* n_groups, uint32_t* n_seqs, uint64_t* n_words, void* hip_stream) {
    if (!e || !groups || !cuts || !n_groups || !n_seqs || !n_words || cuts->window == 0u) return CW_E_INVALID;
    *n_groups = 0; *n_seqs = 0; *n_words = 0;
    std::lock_guard<std::mutex> lk(e->mu);
    if (groups->n_windows > max_batch_windows(e->tmax_plan)) return CW_E_INVALID;
    if (groups->n_seqs != 0 && groups->n_windows == 0) return CW_E_INVALID;
    CW_HIP(hipSetDevice(e->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : e->stream;
    if (groups->n_seqs == 0) { /* groups of none only: no output group */
        if (grp_first) CW_HIP(hipMemsetAsync(grp_first, 0, (size_t)(groups->n_windows + 1) * 4, st));
        if (win_first_seq) CW_HIP(hipMemsetAsync(win_first_seq, 0, 4, st));
        return CW_OK;
    }
    if (!rows || !cuts->cuts || !cuts->cut_off || !groups->win_first_seq || !groups->seq_len || !groups->seq_word_off || !groups->bases) return CW_E_INVALID;
    const uint32_t G = groups->n_windows;
    const uint64_t most = 16ull * groups->n_words / cuts->window + G;
    if (most > 0x7FFFFFFFull) return CW_E_INVALID;
    Layout work;
    const size_t o_grp = work.put((size_t)(G + 1) * 4), o_ws = work.put((size_t)(most + 1) * 4), o_ww = work.put((size_t)(most + 1) * 8), o_st = work.put(32);
    int rc = ensure(&e->scratch, &e->scratch_bytes, work.bytes);
    if (rc) return rc;
    e->last_windows = 0; /* the scratch no longer holds a window or POA run's records (run_sw_locked) */
    uint8_t* base = (uint8_t*)e->scratch;
    CW_HIP(hipMemsetAsync(base + o_st, 0, 32, st));
    CutGroupArgs a;
    a.b = dev_batch(groups);
    a.rows = rows; a.cuts = cuts->cuts; a.cut_off = cuts->cut_off; a.window = cuts->window; a.out_cap = (uint32_t)most;
    a.grp = (uint32_t*)(base + o_grp); a.win_seqs = (uint32_t*)(base + o_ws); a.win_words = (uint64_t*)(base + o_ww);
    a.grp_first = grp_first; a.win_first_seq = win_first_seq; a.seq_len = seq_len; a.seq_word_off = seq_word_off; a.bases = bases;
    a.group_cap = group_cap; a.seq_cap = seq_cap; a.word_cap = word_cap; a.status = (uint32_t*)(base + o_st);
    const uint32_t wgs = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((most + 1 + 3) / 4, (uint64_t)e->cus * 8u));
    cw_cut_index_kernel<<<1, 1024, 0, st>>>(a);
    cw_cut_count_kernel<<<wgs, 256, 0, st>>>(a);
    cw_cut_scan_kernel<<<1, 1024, 0, st>>>(a);
    uint32_t flags[8] = {0, 0, 0, 0, 0, 0, 0, 0}; /* the two flags, then the totals the scan left: groups, sequences, words (64 bits) */
    CW_HIP(hipMemcpyAsync(flags, a.status, 32, hipMemcpyDeviceToHost, st));
    CW_HIP(hipStreamSynchronize(st));
    if (flags[1]) return CW_E_INVALID; /* more windows than the batch's words hold bases for: a malformed batch */
    const uint32_t tot_g = flags[2], tot_s = flags[3];
    uint64_t tot_w = 0;
    memcpy(&tot_w, flags + 4, 8);
    *n_groups = tot_g; *n_seqs = tot_s; *n_words = tot_w;
    if (tot_g > group_cap || tot_s > seq_cap || tot_w > word_cap || !grp_first || !win_first_seq || !seq_len || !seq_word_off || !bases) return CW_E_CAPACITY;
    cw_cut_fill_kernel<<<wgs, 256, 0, st>>>(a);
    CW_HIP(hipGetLastError());
    return CW_OK;
}

/* Debug/inspection (cw_private.h): what plan_sw_path would allocate, part by part, and its grids (host arithmetic only). */
int cw_debug_sw_path_plan(uint32_t n_groups, uint32_t n_seqs, uint64_t n_words, int cus, uint32_t flags, uint64_t* out12) {
    if (!out12 || cus < 1 || (flags & ~CW_SW_PATH_EQX)) return CW_E_INVALID;
    const SwPathPlan p = plan_sw_path(n_groups, n_seqs, n_words, cus);
    const uint64_t v[12] = {p.total, (uint64_t)p.gref, (uint64_t)(p.lstate - p.gref), (uint64_t)(p.dir - p.lstate), (uint64_t)(p.steps - p.dir), (uint64_t)(p.total - p.steps),
                            p.wgs0, p.wgs1, p.wgs_long, p.dir_waves, p.dir_bytes, CW_SW_STEP_BYTES};
    for (int i = 0; i < 12; ++i) out12[i] = v[i];
    return CW_OK;
}

/* Debug/inspection (cw_private.h): what plan_sw would allocate, part by part, and its grids (host arithmetic only). */
int cw_debug_sw_plan(uint32_t n_groups, uint32_t n_seqs, uint64_t n_words, int cus, uint32_t flags, uint64_t* out10) {
    if (!out10 || cus < 1 || (flags & ~CW_SW_WANT_INDELS)) return CW_E_INVALID;
    const SwPlan p = plan_sw(n_groups, n_seqs, n_words, cus, flags);
    const uint64_t v[10] = {p.total, (uint64_t)p.gref, (uint64_t)(p.lstate - p.gref), (uint64_t)(p.dir - p.lstate), (uint64_t)(p.total - p.dir),
                            p.wgs0, p.wgs1, p.wgs_long, p.dir_waves, p.dir_bytes};
    for (int i = 0; i < 10; ++i) out10[i] = v[i];
    return CW_OK;
}

/* Debug/inspection (cw_private.h): what plan_poa would allocate, component by component (host arithmetic only). */
int cw_debug_poa_plan(uint32_t n_groups, uint32_t n_seqs, uint64_t n_words, int cus, uint64_t* out15) {
    if (!out15 || !n_groups || cus < 1) return CW_E_INVALID;
    const ScratchPlan p = plan_poa(n_groups, n_seqs, n_words, cus, 64);
    if (p.arena_cap > 0xFFFFFFFFull) return CW_E_INVALID; /* what cw_poa_run refuses before anything is launched */
    auto slab = [&](int t) { return (uint64_t)p.tier[t].slots * p.tier[t].slab_bytes; };
    const uint64_t v[15] = {p.total, (uint64_t)n_groups * sizeof(WinInfo), (uint64_t)(p.seg_off - p.solid_key), p.seg_cap * 8, p.arena_cap,
                            ((uint64_t)p.task_cap + 1) * sizeof(PoaTask) + (uint64_t)p.member_cap * sizeof(PoaMember), (uint64_t)p.task_cap * 4 * 2 * CW_TIERS,
                            slab(0), slab(1), slab(2), slab(3), slab(4), (uint64_t)p.ablock - p.qslab, (uint64_t)(p.pfall - p.ablock),
                            (uint64_t)(p.sbusy[0] - p.pfall) + (uint64_t)(p.tdbg - p.exg) + (uint64_t)(p.total - p.finvis)};
    for (int i = 0; i < 15; ++i) out15[i] = v[i];
    return CW_OK;
}

uint32_t cw_plan_max_batch_windows(uint32_t k, uint32_t max_template_len) {
    const uint32_t t = plan_tmax(k ? k : 1u, max_template_len);
    return max_batch_windows(t < (uint32_t)CW_TMAX ? t : (uint32_t)CW_TMAX);
}

uint32_t cw_max_batch_windows(cw_engine* e) {
    if (!e) return 0;
    std::lock_guard<std::mutex> lk(e->mu);
    return max_batch_windows(e->tmax_plan);
}

/* Templates longer than the default plan provides for (include/consent_amd.h): the scratch plan and the chain kernel's instance follow; takes effect with
   the engine's next run. */
int cw_configure(cw_engine* e, uint32_t max_template_len) {
    if (!e) return CW_E_INVALID;
    std::lock_guard<std::mutex> lk(e->mu);
    /* (a caller that knows its windows are shorter than the default plan assumes -- the native driver: `-l 500` is 492 k-mers -- gets the smaller
       plan: anchor blocks, segment slots and the arena go by this number, at least 128) */
    const uint32_t kmers = plan_tmax(e->prm.k ? e->prm.k : 1u, max_template_len);
    if (kmers > (uint32_t)CW_TMAX) return CW_E_INVALID; /* beyond what the index kernel holds (CW_WHY_TEMPLATE) */
    e->tmax_plan = kmers;
    return CW_OK;
}

int cw_poll(cw_engine* e) {
    if (!e) return CW_E_INVALID;
    std::lock_guard<std::mutex> lk(e->mu);
    if (!e->timings_valid) return 1;
    if (hipSetDevice(e->device) != hipSuccess) return CW_E_NO_DEVICE;
    hipError_t q = hipEventQuery(e->ev_end);
    if (q == hipSuccess) return 1;
    if (q != hipErrorNotReady) { (void)hipGetLastError(); return CW_E_NO_DEVICE; }
    /* still running: has it left the part that fills the GPU?  (tiers S, M1 and M2 done; what is left is tier L's long tasks, a
       handful of waves, and the finish kernel) */
    int bulk = 0, done = 0;
    for (int i = 0; i < e->n_stages; ++i) {
        const char* n = e->stage_name[i];
        if (strcmp(n, "poa") && strcmp(n, "poa_m1") && strcmp(n, "poa_m2") && strcmp(n, "poa_h")) continue;
        ++bulk;
        q = hipEventQuery(e->ev1[i]);
        if (q == hipSuccess) ++done;
        else if (q != hipErrorNotReady) { (void)hipGetLastError(); return CW_E_NO_DEVICE; }
    }
    return bulk && done == bulk ? 2 : 0;
}

int cw_last_timings(cw_engine* e, float* ms, const char** names, int cap, int* n_stages) {
    if (!e || !n_stages) return CW_E_INVALID;
    *n_stages = 0;
    std::lock_guard<std::mutex> lk(e->mu);
    if (!e->timings_valid) return CW_OK;
    CW_HIP(hipSetDevice(e->device));
    CW_HIP(hipEventSynchronize(e->ev_end));
    int k = 0;
    for (int i = 0; i < e->n_stages && k < cap; ++i, ++k) {
        float t = 0.f;
        CW_HIP(hipEventElapsedTime(&t, e->ev0[i], e->ev1[i]));
        if (ms) ms[k] = t;
        if (names) names[k] = e->stage_name[i];
    }
    if (k < cap) { /* wall time of the whole run on the launch stream (tiers overlap, so this is not the sum) */
        float t = 0.f;
        CW_HIP(hipEventElapsedTime(&t, e->ev_begin, e->ev_end));
        if (ms) ms[k] = t;
        if (names) names[k] = "total";
        ++k;
    }
    *n_stages = k;
    return CW_OK;
}

/* Debug/inspection (cw_private.h): what plan_scratch would allocate, component by component (host arithmetic only). */
int cw_debug_plan(uint32_t k, uint32_t solid, uint32_t n_windows, uint32_t n_seqs, uint64_t n_words, int cus, uint32_t scale, uint32_t tmax, uint64_t* out15) {
    if (!out15 || !n_windows || !solid) return CW_E_INVALID;
    cw_params prm{k, solid, 8, 2, 150};
    const ScratchPlan p = plan_scratch(PlanInput{prm, n_windows, n_seqs, n_words, cus, 64, scale ? scale : 1, tmax ? tmax : 1024, false});
    auto slab = [&](int t) { return (uint64_t)p.tier[t].slots * p.tier[t].slab_bytes; };
    const uint64_t v[15] = {p.total, (uint64_t)n_windows * sizeof(WinInfo), p.solid_cap * 8, p.seg_cap * 8, p.arena_cap,
                            ((uint64_t)p.task_cap + 1) * sizeof(PoaTask) + (uint64_t)p.member_cap * sizeof(PoaMember), (uint64_t)p.task_cap * 4 * 2 * CW_TIERS,
                            slab(0), slab(1), slab(2), slab(3), slab(4), (uint64_t)p.hslab - p.qslab + ((uint64_t)p.ablock - p.hslab), p.ablock_units * 16,
                            (uint64_t)(p.exg - p.pfall) + (uint64_t)(p.tdbg - p.exg)};
    for (int i = 0; i < 15; ++i) out15[i] = v[i];
    return CW_OK;
}

/* Debug/inspection (cw_private.h): the capacities of that plan and the batch limit of its tmax (host arithmetic only). */
int cw_debug_plan_caps(uint32_t k, uint32_t solid, uint32_t n_windows, uint32_t n_seqs, uint64_t n_words, int cus, uint32_t scale, uint32_t tmax, int pf_full, uint64_t* out8) {
    if (!out8 || !n_windows || !solid) return CW_E_INVALID;
    cw_params prm{k, solid, 8, 2, 150};
    const uint32_t t = tmax ? tmax : 1024;
    const ScratchPlan p = plan_scratch(PlanInput{prm, n_windows, n_seqs, n_words, cus, 64, scale ? scale : 1, t, pf_full != 0});
    const uint64_t v[8] = {p.total, p.solid_cap, p.seg_cap, p.arena_cap, p.arena_scale, p.pfall_elems / t, max_batch_windows(t), p.task_cap};
    for (int i = 0; i < 8; ++i) out8[i] = v[i];
    return CW_OK;
}

/* Debug/inspection (cw_private.h): copy the engine's per-window bookkeeping of the last run (16 u32 per window) to host. */
int cw_debug_win_info(cw_engine* e, uint32_t n_windows, uint32_t* out16) {
    if (!e || !out16 || !e->scratch) return CW_E_INVALID;
    std::lock_guard<std::mutex> lk(e->mu);
    if (n_windows > e->last_windows) return CW_E_INVALID;
    CW_HIP(hipSetDevice(e->device));
    CW_HIP(hipDeviceSynchronize());
    CW_HIP(hipMemcpy(out16, e->scratch, (size_t)n_windows * sizeof(WinInfo), hipMemcpyDeviceToHost));
    return CW_OK;
}

/* Debug/inspection (cw_private.h): the index kernel's count table of one window of the last run -- its slice of solid_key / solid_cnt (WinInfo::solid_base,
 * n_solid): the ascending solid k-mers and their exact pile-wide counts.  *n = the entries the window has; the first min(*n, cap) are copied. */
int cw_debug_solid_table(cw_engine* e, uint32_t window, uint32_t* keys, uint32_t* counts, uint32_t cap, uint32_t* n) {
    if (!e || !e->scratch || !n || (cap && (!keys || !counts))) return CW_E_INVALID;
    std::lock_guard<std::mutex> lk(e->mu);
    if (window >= e->last_windows) return CW_E_INVALID;
    CW_HIP(hipSetDevice(e->device));
    CW_HIP(hipDeviceSynchronize());
    WinInfo wi;
    CW_HIP(hipMemcpy(&wi, (const uint8_t*)e->scratch + (size_t)window * sizeof(WinInfo), sizeof(wi), hipMemcpyDeviceToHost));
    if (wi.n_solid > wi.solid_cap) return CW_E_INVALID; /* (never: the index kernel writes n_solid only when the set fits) */
    *n = wi.n_solid;
    const size_t take = wi.n_solid < cap ? wi.n_solid : cap;
    if (take) {
        CW_HIP(hipMemcpy(keys, (const uint8_t*)e->scratch + e->last_solid_key_off + (size_t)wi.solid_base * 4, take * 4, hipMemcpyDeviceToHost));
        CW_HIP(hipMemcpy(counts, (const uint8_t*)e->scratch + e->last_solid_cnt_off + (size_t)wi.solid_base * 4, take * 4, hipMemcpyDeviceToHost));
    }
    return CW_OK;
}

/* Debug/inspection (cw_private.h): the anchor block of one window of the last run, as idx_hand_over left it (cw_index.h CwAbCarve) -- the window's slice of
 * the scratch plan's ablock region (WinInfo::ab_base, ab_cap), which nothing else lies in and which cw_chain_kernel only reads.  *n = cw_ab_bytes of the
 * block's own header; the first min(*n, cap) bytes are copied. */
int cw_debug_anchor_block(cw_engine* e, uint32_t window, uint8_t* out, uint64_t cap, uint64_t* n) {
    if (!e || !e->scratch || !n || (cap && !out)) return CW_E_INVALID;
    std::lock_guard<std::mutex> lk(e->mu);
    if (window >= e->last_windows) return CW_E_INVALID;
    CW_HIP(hipSetDevice(e->device));
    CW_HIP(hipDeviceSynchronize());
    WinInfo wi;
    CW_HIP(hipMemcpy(&wi, (const uint8_t*)e->scratch + (size_t)window * sizeof(WinInfo), sizeof(wi), hipMemcpyDeviceToHost));
    /* no block: a POA-only run, a window without a template k-mer, or one the setup or index phase stopped (the later phases stop a window behind its block) */
    if (wi.ab_cap == 0 || wi.status == CW_WIN_TEMPLATE) return CW_E_INVALID;
    if (wi.status == CW_WIN_OVERFLOW && (wi.pad_ == CW_WHY_SETUP || wi.pad_ == CW_WHY_COUNT || wi.pad_ == CW_WHY_SOLIDCAP || wi.pad_ == CW_WHY_TEMPLATE || wi.pad_ == CW_WHY_MATRIX)) return CW_E_INVALID;
    if ((uint64_t)wi.ab_base + wi.ab_cap > e->last_ablock_units) return CW_E_INVALID; /* (never: cw_setup_kernel stops such a window) */
    const uint8_t* blk = (const uint8_t*)e->scratch + e->last_ablock_off + ((size_t)wi.ab_base << 4);
    uint32_t hdr[5];
    CW_HIP(hipMemcpy(hdr, blk, sizeof(hdr), hipMemcpyDeviceToHost));
    const uint64_t bytes = cw_ab_bytes(hdr[0], hdr[1], hdr[2], hdr[4]);
    if (bytes > ((uint64_t)wi.ab_cap << 4)) return CW_E_INVALID;
    *n = bytes;
    const uint64_t take = bytes < cap ? bytes : cap;
    if (take) CW_HIP(hipMemcpy(out, blk, (size_t)take, hipMemcpyDeviceToHost));
    return CW_OK;
}

/* Debug/inspection (cw_private.h): the nine offsets of cw_ab_carve<uint64_t>(0, ...), in the order of CwAbCarve (host arithmetic only). */
int cw_debug_ab_layout(uint32_t A, uint32_t N, uint32_t n_dirty, uint32_t n_rows, uint64_t* out9) {
    if (!out9) return CW_E_INVALID;
    const CwAbCarve<uint64_t> c = cw_ab_carve<uint64_t>(0, A, N, n_dirty, n_rows);
    const uint64_t v[9] = {c.hdr, c.ckey, c.pres, c.dirty, c.badm, c.rowid, c.delta, c.P, c.end};
    for (int i = 0; i < 9; ++i) out9[i] = v[i];
    return CW_OK;
}

/* Debug/inspection (cw_private.h): the segmentation of one window of the last run -- WinInfo::n_segs, the window's slots of seg_len, and the task records
 * that name the window with their members.  Host code only: the task and member arrays are read as the chain kernel (cw_poa_tasks_kernel in an operator
 * run) left them -- the tiers read the fields returned here and rewrite none of them (PoaTask::state, which they do rewrite, is not returned); seg_len of
 * a task's slot is the tier's output. */
int cw_debug_segments(cw_engine* e, uint32_t window, uint32_t* n_segs, uint32_t* seg_len, uint32_t seg_cap, uint32_t* tasks4, uint32_t task_cap, uint32_t* n_tasks,
                      uint32_t* members3, uint32_t member_cap, uint32_t* n_members) {
    if (!e || !e->scratch || !n_segs || !n_tasks || !n_members || (seg_cap && !seg_len) || (task_cap && !tasks4) || (member_cap && !members3)) return CW_E_INVALID;
    std::lock_guard<std::mutex> lk(e->mu);
    if (window >= e->last_windows || !e->last_win_first_seq) return CW_E_INVALID;
    BatchCounters c;
    if (int rc = read_counters_idle(e, &c)) return rc;
    const uint8_t* base = (const uint8_t*)e->scratch;
    WinInfo wi;
    uint32_t s0 = 0;
    CW_HIP(hipMemcpy(&wi, base + (size_t)window * sizeof(WinInfo), sizeof(wi), hipMemcpyDeviceToHost));
    CW_HIP(hipMemcpy(&s0, e->last_win_first_seq + window, 4, hipMemcpyDeviceToHost));
    if (wi.n_segs > wi.seg_cap) return CW_E_INVALID; /* (never: the chain kernel writes n_segs only when the segments fit) */
    *n_segs = wi.n_segs;
    const size_t take = wi.n_segs < seg_cap ? wi.n_segs : seg_cap;
    if (take) CW_HIP(hipMemcpy(seg_len, base + e->last_seg_len_off + (size_t)wi.seg_base * 4, take * 4, hipMemcpyDeviceToHost));
    const uint32_t nt = c.n_tasks < e->last_task_cap ? c.n_tasks : e->last_task_cap; /* the counter runs on when a capacity stops a window: clamped, as the tiers clamp it */
    std::vector<PoaTask> tasks(nt);
    if (nt) CW_HIP(hipMemcpy(tasks.data(), base + e->last_tasks_off, (size_t)nt * sizeof(PoaTask), hipMemcpyDeviceToHost));
    uint32_t found = 0, mem = 0;
    std::vector<PoaMember> pm;
    for (uint32_t t = 0; t < nt; ++t) {
        const PoaTask& tk = tasks[t];
        if (tk.window != window) continue;
        if (found < task_cap) { uint32_t* o = tasks4 + (size_t)found * 4; o[0] = tk.seg_slot - wi.seg_base; o[1] = tk.n_members; o[2] = tk.max_len & 0xFFFFu; o[3] = mem; }
        if (tk.n_members && mem < member_cap) {
            const uint32_t n = tk.n_members < member_cap - mem ? tk.n_members : member_cap - mem;
            pm.resize(n);
            CW_HIP(hipMemcpy(pm.data(), base + e->last_members_off + (size_t)tk.member_off * sizeof(PoaMember), (size_t)n * sizeof(PoaMember), hipMemcpyDeviceToHost));
            for (uint32_t i = 0; i < n; ++i) { uint32_t* o = members3 + (size_t)(mem + i) * 3; o[0] = pm[i].seq - s0; o[1] = pm[i].start; o[2] = pm[i].len; }
        }
        found++; mem += tk.n_members;
    }
    *n_tasks = found; *n_members = mem;
    return CW_OK;
}

/* Debug/inspection (cw_private.h): the batch counters (u32) and the per-phase cycle totals (u64) of the last run; the caller says how many
 * words each of its buffers holds and gets min(capacity, available) of them (returned through the two *_n when given). */
int cw_debug_profile(cw_engine* e, uint32_t* counters, uint32_t counters_cap, unsigned long long* prof, uint32_t prof_cap, uint32_t* counters_n, uint32_t* prof_n) {
    if (!e || !e->scratch || !counters || !prof) return CW_E_INVALID;
    std::lock_guard<std::mutex> lk(e->mu);
    BatchCounters c;
    if (int rc = read_counters_idle(e, &c)) return rc;
    const uint32_t nc = counters_cap < 6u + 4u * CW_TIERS ? counters_cap : 6u + 4u * CW_TIERS; /* n_tasks .. any_overflow, then n_tier, next_tier, n_over, next_over [CW_TIERS] each */
    const uint32_t np = prof_cap < (uint32_t)CW_PROF_SLOTS ? prof_cap : (uint32_t)CW_PROF_SLOTS;
    memcpy(counters, &c, (size_t)nc * 4);
    memcpy(prof, c.prof, (size_t)np * sizeof(unsigned long long));
    if (counters_n) *counters_n = nc;
    if (prof_n) *prof_n = np;
    return CW_OK;
}

/* Debug/inspection (cw_private.h): tier X's counters of the last run -- routed, done, stopped, largest cell count (BatchCounters::x_*) */
int cw_debug_tier_x(cw_engine* e, uint32_t* out4) {
    if (!e || !e->scratch || !out4) return CW_E_INVALID;
    std::lock_guard<std::mutex> lk(e->mu);
    BatchCounters c;
    if (int rc = read_counters_idle(e, &c)) return rc;
    out4[0] = c.x_routed; out4[1] = c.x_done; out4[2] = c.x_stopped; out4[3] = c.x_cells;
    return CW_OK;
}

/* Debug/inspection (cw_private.h): tier Q's two ranges in the last run -- long entries of its list (BatchCounters::q_split), short tasks the eight-lane loop
 * finished, short tasks it handed on to tier S.  A build without the eight-lane loop reports every entry as long. */
int cw_debug_tier_q(cw_engine* e, uint32_t* out3) {
    if (!e || !e->scratch || !out3) return CW_E_INVALID;
    std::lock_guard<std::mutex> lk(e->mu);
    BatchCounters c;
    if (int rc = read_counters_idle(e, &c)) return rc;
    out3[0] = c.q_split; out3[1] = c.q_short_done; out3[2] = c.q_short_on;
    return CW_OK;
}

/* Debug/inspection (cw_private.h): one routed list of the last run after the tier sort, the same list as it was emitted where the run kept it, and the batch's
 * task records.  Host code only. */
int cw_debug_tier_lists(cw_engine* e, uint32_t list, uint32_t* sorted, uint32_t* emitted, uint32_t cap, uint32_t* n, uint32_t* kept, uint32_t* tasks4, uint32_t task_cap,
                        uint32_t* n_tasks) {
    if (!e || !e->scratch || !n || !kept || !n_tasks || list >= (uint32_t)CW_TIERS || list == (uint32_t)CW_POAX_LIST || (cap && (!sorted || !emitted)) || (task_cap && !tasks4)) return CW_E_INVALID;
    std::lock_guard<std::mutex> lk(e->mu);
    BatchCounters c;
    if (int rc = read_counters_idle(e, &c)) return rc;
    const uint8_t* base = (const uint8_t*)e->scratch;
    const uint32_t have = c.n_tier[list] < e->last_task_cap ? c.n_tier[list] : e->last_task_cap; /* clamped, as the sort and the tiers clamp it */
    *n = have; *kept = e->emitted_cap ? 1u : 0u;
    const uint32_t take = have < cap ? have : cap;
    if (take) CW_HIP(hipMemcpy(sorted, base + e->last_list_off[list], (size_t)take * 4, hipMemcpyDeviceToHost));
    if (take && e->emitted_cap) CW_HIP(hipMemcpy(emitted, (const uint32_t*)e->emitted + (size_t)list * e->emitted_cap, (size_t)take * 4, hipMemcpyDeviceToHost));
    const uint32_t nt = c.n_tasks < e->last_task_cap ? c.n_tasks : e->last_task_cap;
    *n_tasks = nt;
    const uint32_t tt = nt < task_cap ? nt : task_cap;
    std::vector<PoaTask> tasks(tt);
    if (tt) CW_HIP(hipMemcpy(tasks.data(), base + e->last_tasks_off, (size_t)tt * sizeof(PoaTask), hipMemcpyDeviceToHost));
    for (uint32_t t = 0; t < tt; ++t) { uint32_t* o = tasks4 + (size_t)t * 4; o[0] = tasks[t].window; o[1] = tasks[t].seg_slot; o[2] = tasks[t].n_members; o[3] = tasks[t].max_len; }
    return CW_OK;
}

/* Debug/inspection (cw_private.h): with CW_TASK_TRACE set, 12 words per POA task of the last run: the PoaTask record (window, seg_slot,
 * member_off, n_members, max_len, out_off, out_cap, state) + start and duration in 10 ns units, tier | rc << 8 | pass << 16, wave */
int cw_debug_task_trace(cw_engine* e, uint32_t cap_tasks, uint32_t* out12, uint32_t* n_tasks) {
    if (!e || !e->scratch || !out12 || !n_tasks || !getenv("CW_TASK_TRACE")) return CW_E_INVALID;
    std::lock_guard<std::mutex> lk(e->mu);
    BatchCounters c;
    if (int rc = read_counters_idle(e, &c)) return rc;
    uint32_t n = c.n_tasks < e->last_task_cap ? c.n_tasks : e->last_task_cap;
    if (n > cap_tasks) n = cap_tasks;
    std::vector<uint32_t> a((size_t)n * 8), d((size_t)n * 4);
    CW_HIP(hipMemcpy(a.data(), (uint8_t*)e->scratch + e->last_tasks_off, (size_t)n * 32, hipMemcpyDeviceToHost));
    CW_HIP(hipMemcpy(d.data(), (uint8_t*)e->scratch + e->last_tdbg_off, (size_t)n * 16, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < n; ++i) { memcpy(out12 + (size_t)i * 12, &a[(size_t)i * 8], 32); memcpy(out12 + (size_t)i * 12 + 8, &d[(size_t)i * 4], 16); }
    *n_tasks = n;
    return CW_OK;
}

int cw_extract_piles_device(cw_engine* e, const cw_read_set* reads, const cw_overlap* overlaps, uint64_t n_overlaps,
                            const cw_window_job* jobs, uint32_t n_jobs, uint32_t k, uint32_t* win_first_seq, uint32_t* seq_len,
                            uint64_t* seq_word_off, uint32_t* bases, uint32_t seq_cap, uint64_t word_cap, uint32_t* n_seqs,
                            uint64_t* n_words, void* hip_stream) {
    return cw_extract_impl(e, reads, overlaps, n_overlaps, jobs, nullptr, n_jobs, k, win_first_seq, seq_len, seq_word_off, bases, seq_cap, word_cap, n_seqs,
                           n_words, hip_stream);
}

/* jobs_host: the same jobs in host memory when the caller has them (the library's own driver does): saves the device-to-host copy */
int cw_extract_impl(cw_engine* e, const cw_read_set* reads, const cw_overlap* overlaps, uint64_t n_overlaps, const cw_window_job* jobs,
                    const cw_window_job* jobs_host, uint32_t n_jobs, uint32_t k, uint32_t* win_first_seq, uint32_t* seq_len, uint64_t* seq_word_off,
                    uint32_t* bases, uint32_t seq_cap, uint64_t word_cap, uint32_t* n_seqs, uint64_t* n_words, void* hip_stream) {
    if (!e || !reads || !jobs || !n_seqs || !n_words || (n_overlaps && !overlaps) || k < 1) return CW_E_INVALID;
    *n_seqs = 0; *n_words = 0;
    if (n_jobs == 0) return CW_OK;
    std::lock_guard<std::mutex> lk(e->mu);
    CW_HIP(hipSetDevice(e->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : e->stream;
    /* per-window descriptor offsets need the jobs' overlap counts: take them from the device once */
    std::vector<cw_window_job> hj_own;
    std::vector<uint64_t> doff;
    try { if (!jobs_host) hj_own.resize(n_jobs); doff.assign((size_t)n_jobs + 1, 0); } catch (...) { return CW_E_NOMEM; }
    if (!jobs_host) {
        CW_HIP(hipMemcpyAsync(hj_own.data(), jobs, (size_t)n_jobs * sizeof(cw_window_job), hipMemcpyDeviceToHost, st));
        CW_HIP(hipStreamSynchronize(st));
    }
    const cw_window_job* hj = jobs_host ? jobs_host : hj_own.data();
    for (uint32_t w = 0; w < n_jobs; ++w) {
        if ((uint64_t)hj[w].ovl_first + hj[w].ovl_count > n_overlaps || hj[w].tpl_read >= reads->n_reads || hj[w].q_end < hj[w].q_beg) return CW_E_INVALID;
        doff[w + 1] = doff[w] + hj[w].ovl_count;
    }
    Layout work;
    const size_t o_desc = work.put((size_t)doff[n_jobs] * sizeof(ExtractDesc) + 16), o_doff = work.put((size_t)(n_jobs + 1) * 8),
                 o_ws = work.put((size_t)(n_jobs + 1) * 4), o_ww = work.put((size_t)(n_jobs + 1) * 8), o_st = work.put(16);
    int rc = ensure(&e->xscratch, &e->xscratch_bytes, work.bytes);
    if (rc) return rc;
    uint8_t* base = (uint8_t*)e->xscratch;
    CW_HIP(hipMemcpyAsync(base + o_doff, doff.data(), (size_t)(n_jobs + 1) * 8, hipMemcpyHostToDevice, st));
    CW_HIP(hipMemsetAsync(base + o_st, 0, 16, st));
    ExtractArgs a;
    a.reads = *reads; a.ovl = overlaps; a.jobs = jobs; a.n_jobs = n_jobs; a.k = k;
    a.desc = (ExtractDesc*)(base + o_desc); a.desc_off = (const uint64_t*)(base + o_doff);
    a.win_seqs = (uint32_t*)(base + o_ws); a.win_words = (uint64_t*)(base + o_ww);
    a.win_first_seq = win_first_seq; a.seq_len = seq_len; a.seq_word_off = seq_word_off; a.bases = bases;
    a.seq_cap = seq_cap; a.word_cap = word_cap; a.status = (uint32_t*)(base + o_st);
    cw_extract_count_kernel<<<(n_jobs + 3) / 4, 256, 0, st>>>(a);
    cw_extract_scan_kernel<<<1, 1024, 0, st>>>(a);
    uint32_t tot_s = 0, flags[4] = {0, 0, 0, 0}; uint64_t tot_w = 0;
    CW_HIP(hipMemcpyAsync(&tot_s, a.win_seqs + n_jobs, 4, hipMemcpyDeviceToHost, st));
    CW_HIP(hipMemcpyAsync(&tot_w, a.win_words + n_jobs, 8, hipMemcpyDeviceToHost, st));
    CW_HIP(hipMemcpyAsync(flags, a.status, 16, hipMemcpyDeviceToHost, st));
    CW_HIP(hipStreamSynchronize(st));
    *n_seqs = tot_s; *n_words = tot_w;
    if (flags[2]) return CW_E_INVALID;  /* an overlap names a target read outside the read set */
    if (flags[1]) return CW_E_CAPACITY; /* a piece longer than 65535 bases (the batch format's length limit): an error, never a silently shorter pile */
    if (tot_s > seq_cap || tot_w > word_cap || !win_first_seq || !seq_len || !seq_word_off || !bases) return CW_E_CAPACITY;
    cw_extract_fill_kernel<<<(n_jobs + 1 + 3) / 4, 256, 0, st>>>(a);
    CW_HIP(hipGetLastError());
    return CW_OK;
}

__global__ void __launch_bounds__(256) cw_add_offsets_kernel(uint32_t* a32, uint64_t n32, uint32_t add32, uint64_t* a64, uint64_t n64, uint64_t add64) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i < n32) a32[i] += add32;
    if (i < n64) a64[i] += add64;
}

int cw_add_offsets_device(uint32_t* a32, uint64_t n32, uint32_t add32, uint64_t* a64, uint64_t n64, uint64_t add64, void* hip_stream) {
    if ((n32 && !a32) || (n64 && !a64)) return CW_E_INVALID;
    const uint64_t n = n32 > n64 ? n32 : n64;
    if (n == 0 || (add32 == 0 && add64 == 0)) return CW_OK;
    if ((n + 255) / 256 > 0x7FFFFFFFull) return CW_E_INVALID;
    cw_add_offsets_kernel<<<(uint32_t)((n + 255) / 256), 256, 0, (hipStream_t)hip_stream>>>(a32, n32, add32, a64, n64, add64);
    CW_HIP(hipGetLastError());
    return CW_OK;
}

int cw_plan_results_device(cw_engine* e, const cw_batch* batch, uint64_t* cons_off, uint64_t* solid_off, uint64_t* cons_total, uint64_t* solid_total,
                           void* hip_stream) {
    if (!e || !batch || !cons_off || !solid_off || !cons_total || !solid_total) return CW_E_INVALID;
    *cons_total = 0; *solid_total = 0;
    if (batch->n_windows == 0) return CW_OK;
    if (!batch->win_first_seq || !batch->seq_len) return CW_E_INVALID;
    std::lock_guard<std::mutex> lk(e->mu);
    CW_HIP(hipSetDevice(e->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : e->stream;
    int rc = ensure(&e->xscratch, &e->xscratch_bytes, 256);
    if (rc) return rc;
    PlanArgs a;
    a.n_windows = batch->n_windows; a.k = e->prm.k; a.solid = e->prm.solid;
    a.win_first_seq = batch->win_first_seq; a.seq_len = batch->seq_len;
    a.cons_off = cons_off; a.solid_off = solid_off; a.totals = (uint64_t*)e->xscratch;
    cw_plan_need_kernel<<<(batch->n_windows + 3) / 4, 256, 0, st>>>(a);
    cw_plan_scan_kernel<<<1, 1024, 0, st>>>(a);
    uint64_t tot[2] = {0, 0};
    CW_HIP(hipMemcpyAsync(tot, a.totals, 16, hipMemcpyDeviceToHost, st));
    CW_HIP(hipStreamSynchronize(st));
    *cons_total = tot[0]; *solid_total = tot[1];
    return CW_OK;
}

int cw_stitch_device(cw_engine* e, const cw_read_set* reads, const cw_stitch_read* jobs, uint32_t n_reads, const uint32_t* win_pos,
                     const cw_batch* batch, const cw_result* res, uint32_t window_size, uint32_t window_overlap, int32_t do_trim,
                     char* out, const uint64_t* out_off, uint32_t* out_len, uint8_t* read_status, void* hip_stream) {
    if (!e || !reads || !batch || !res || !out_off || !out_len || !read_status) return CW_E_INVALID;
    if (n_reads == 0) return CW_OK;
    if (!jobs || !win_pos || !out || !res->cons || !res->cons_off || !res->cons_len || !res->win_status || !res->solid || !res->solid_off ||
        !res->solid_len || !batch->win_first_seq || !batch->seq_len || !batch->seq_word_off || !batch->bases)
        return CW_E_INVALID;
    if ((uint64_t)window_size + 2ull * window_overlap > CW_ST_RMAX) return CW_E_INVALID;
    std::lock_guard<std::mutex> lk(e->mu);
    CW_HIP(hipSetDevice(e->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : e->stream;
    const bool want_trace = CW_AID_ENV("CW_STITCH_TRACE") != nullptr;
    const size_t trace_bytes = want_trace ? (size_t)batch->n_windows * 32 : 0;
#if CW_ST_WITNESS /* the route witness (cw_stitch.h CwStRoute): its records lie behind the order */
    const size_t route_bytes = want_trace ? ((size_t)batch->n_windows * CW_ST_WIT_WORDS + n_reads) * 4 : 0;
#else
    const size_t route_bytes = 0;
#endif
    int rc = ensure(&e->xscratch, &e->xscratch_bytes, 256 + trace_bytes + (size_t)n_reads * 4 + route_bytes);
    if (rc) return rc;
    e->stitch_route_off = 0;
    CW_HIP(hipMemsetAsync(e->xscratch, 0, 16, st)); /* a.cursor: three words (cw_stitch.h) */
    StitchArgs a;
    a.order = (uint32_t*)((uint8_t*)e->xscratch + 256 + trace_bytes);
    a.trace = want_trace ? (uint32_t*)((uint8_t*)e->xscratch + 256) : nullptr;
    if (want_trace) CW_HIP(hipMemsetAsync(a.trace, 0xFF, (size_t)batch->n_windows * 32, st));
#if CW_ST_WITNESS
    if (want_trace) {
        e->stitch_route_off = 256 + trace_bytes + (size_t)n_reads * 4;
        a.route = (uint32_t*)((uint8_t*)e->xscratch + e->stitch_route_off);
        a.read_route = a.route + (size_t)batch->n_windows * CW_ST_WIT_WORDS;
        CW_HIP(hipMemsetAsync(a.route, 0xFF, route_bytes, st));
    }
#endif
    a.reads = *reads; a.jobs = jobs; a.n_reads = n_reads; a.win_pos = win_pos;
    a.batch.n_windows = batch->n_windows; a.batch.win_first_seq = batch->win_first_seq; a.batch.seq_len = batch->seq_len;
    a.batch.seq_word_off = batch->seq_word_off; a.batch.bases = batch->bases;
    a.cons = res->cons; a.cons_off = res->cons_off; a.cons_len = res->cons_len; a.win_status = res->win_status;
    a.solid = res->solid; a.solid_off = res->solid_off; a.solid_len = res->solid_len;
    a.window_size = window_size; a.window_overlap = window_overlap; a.mer_size = e->prm.k; a.do_trim = do_trim;
    a.out = out; a.out_off = out_off; a.out_len = out_len; a.read_status = read_status; a.cursor = (uint32_t*)e->xscratch;
    /* one work-group of the wide kernel per CU, i.e. one wave per SIMD: the launch lasts as long as its longest read, and that read's wave is
       faster alone on its SIMD (measured with the register count deciding it: 55.3 ms per job at one wave per SIMD, 60.5 at two).  The kernel
       fits two per CU by registers and LDS; asking for more than half of the LDS keeps the second one off (CW_STITCH_TWO_PER_CU=1: don't). */
    const size_t lds_one = CW_AID_ENV("CW_STITCH_TWO_PER_CU") ? 0 : stitch_lds_one(e->prop);
    const size_t lds = kLdsStitch > lds_one ? kLdsStitch : lds_one;
    uint32_t wgs = (n_reads + CW_ST_WAVES - 1) / CW_ST_WAVES;
    if (wgs > CW_ST_MAX_WGS) wgs = CW_ST_MAX_WGS;
    /* test aid: CW_STITCH_DIR_BYTES shrinks the banded-traceback scratch so that the capacity path can be exercised */
    a.dir_bytes = CW_ST_DIR_BYTES;
    if (const char* env = CW_AID_ENV("CW_STITCH_DIR_BYTES")) a.dir_bytes = (uint32_t)strtoul(env, nullptr, 10);
    if (a.dir_bytes < 64) a.dir_bytes = 64;
    /* the last launch (consensuses beyond CW_ST_QMAX characters; one wave per work-group, everything in global memory) has its slabs behind the traceback scratch */
    uint32_t wgs_h = n_reads < CW_STH_MAX_WGS ? n_reads : CW_STH_MAX_WGS;
    if (wgs_h > wgs * CW_ST_WAVES) wgs_h = wgs * CW_ST_WAVES; /* (its waves use the first wgs_h traceback scratches) */
    const size_t dir_total = (((size_t)wgs * CW_ST_WAVES * a.dir_bytes) + 255u) & ~(size_t)255u;
    rc = ensure(&e->stitch_scratch, &e->stitch_scratch_bytes, dir_total + (size_t)wgs_h * CW_STH_WAVE_BYTES);
    if (rc) return rc;
    a.dir_scratch = (int8_t*)e->stitch_scratch;
    a.huge = (uint8_t*)e->stitch_scratch + dir_total;
    a.prio = 1;
    if (const char* env = CW_AID_ENV("CW_STITCH_PRIO")) a.prio = atoi(env); /* measured: 69.6 -> 65.3 ms per job of 32768 windows (E. coli-scale ONT set) */
    cw_stitch_order_kernel<<<1, 1024, 0, st>>>(a);
    cw_stitch_kernel<CW_ST_QMAX, CW_ST_RMAX, 16, CW_ST_WAVES><<<wgs, 64 * CW_ST_WAVES, lds, st>>>(a);
    /* the reads the launch above marked (a window's consensus beyond CW_ST_QMAX characters: normally none, and the waves find nothing to do) */
    cw_stitch_kernel<CW_STH_QMAX, CW_ST_RMAX, 0, 1><<<wgs_h, 64, 0, st>>>(a);
    CW_HIP(hipGetLastError());
    return CW_OK;
}

int cw_debug_stitch_trace(cw_engine* e, uint32_t n_windows, uint32_t* out) {
    if (!e || !out || !e->xscratch || e->xscratch_bytes < 256 + (size_t)n_windows * 32) return CW_E_INVALID;
    std::lock_guard<std::mutex> lk(e->mu);
    CW_HIP(hipSetDevice(e->device));
    CW_HIP(hipDeviceSynchronize());
    CW_HIP(hipMemcpy(out, (uint8_t*)e->xscratch + 256, (size_t)n_windows * 32, hipMemcpyDeviceToHost));
    return CW_OK;
}

int cw_debug_stitch_route(cw_engine* e, uint32_t n_windows, uint32_t n_reads, uint32_t* win_out, uint32_t* read_out) {
    if (!e || !win_out || !read_out) return CW_E_INVALID;
    std::lock_guard<std::mutex> lk(e->mu);
    const size_t off = e->stitch_route_off, win_bytes = (size_t)n_windows * CW_ST_WIT_WORDS * 4;
    if (off == 0) return 0; /* the product library, or a call without CW_STITCH_TRACE: nothing was recorded */
    if (!e->xscratch || e->xscratch_bytes < off + win_bytes + (size_t)n_reads * 4) return CW_E_INVALID;
    CW_HIP(hipSetDevice(e->device));
    CW_HIP(hipDeviceSynchronize());
    CW_HIP(hipMemcpy(win_out, (uint8_t*)e->xscratch + off, win_bytes, hipMemcpyDeviceToHost));
    CW_HIP(hipMemcpy(read_out, (uint8_t*)e->xscratch + off + win_bytes, (size_t)n_reads * 4, hipMemcpyDeviceToHost));
    return 1;
}

/* ---- host batches: cw_submit / cw_wait (and cw_run = both) -------------------------------------------------------------------
 * H2D on its own stream, the kernels on the compute stream, the results compacted on the device (cw_pack_*: only the bytes the
 * windows actually produced cross PCIe, not the capacities the caller reserved), D2H on a third stream into pinned staging, then
 * scattered into the caller's arrays.  With two batches in flight the copies of one overlap the kernels of the other. */
/* pf_full: see run_device_locked (cw_run's re-run after CW_WHY_MATRIX) */
static int submit_locked(cw_engine* e, const cw_batch* b, const cw_result* r, int* ticket, bool pf_full) {
    if (!e || !b || !r || !ticket || !r->cons || !r->cons_off || !r->cons_len || !r->win_status) return CW_E_INVALID;
    *ticket = -1;
    if (b->n_windows && (!b->win_first_seq || !b->seq_len || !b->seq_word_off || !b->bases)) return CW_E_INVALID;
    if (b->n_windows > CW_MAX_BATCH_WINDOWS) return CW_E_INVALID;
    const uint32_t W = b->n_windows, S = b->n_seqs;
    /* light validation of the host batch */
    if (W) {
        if (b->win_first_seq[0] != 0 || b->win_first_seq[W] != S) return CW_E_INVALID;
        for (uint32_t w = 0; w < W; ++w) if (b->win_first_seq[w + 1] < b->win_first_seq[w]) return CW_E_INVALID;
        for (uint32_t s = 0; s < S; ++s)
            if (b->seq_word_off[s] + ((uint64_t)b->seq_len[s] + 15) / 16 > b->n_words || b->seq_len[s] > 65535u) return CW_E_INVALID;
    }
    const bool want_solid = r->solid != nullptr;
    if (want_solid && (!r->solid_off || !r->solid_len)) return CW_E_INVALID;
    std::lock_guard<std::mutex> lk(e->mu);
    if (W > max_batch_windows(e->tmax_plan)) return CW_E_INVALID; /* cw_max_batch_windows: refused before anything is copied or launched */
    /* the copy streams exist only for callers of the host-batch path, and are created after the four kernel streams: the runtime
       multiplexes streams onto a handful of hardware queues in creation order, and two POA tiers that land on one queue run one after
       the other instead of side by side (measured: tier M1 started only when tier M2 had ended) */
    if (!e->copy_in) {
        CW_HIP(hipSetDevice(e->device));
        if (hipStreamCreateWithFlags(&e->copy_in, hipStreamNonBlocking) != hipSuccess) { e->copy_in = nullptr; return CW_E_NO_DEVICE; }
        if (hipStreamCreateWithFlags(&e->copy_out, hipStreamNonBlocking) != hipSuccess) { e->copy_out = nullptr; return CW_E_NO_DEVICE; }
    }
    int si = -1;
    for (int i = 0; i < CW_SLOTS; ++i) if (!e->slot[i].busy) { si = i; break; }
    if (si < 0) return CW_E_INVALID; /* CW_SLOTS batches are in flight already: cw_wait one of them first */
    cw_slot& sl = e->slot[si];
    sl.res = *r; sl.n_windows = W; sl.want_solid = want_solid;
    if (W == 0) { sl.busy = true; sl.waiting = false; *ticket = si; return CW_OK; }
    CW_HIP(hipSetDevice(e->device));

    Layout in, out;
    const size_t i_wfs = in.put((size_t)(W + 1) * 4), i_len = in.put((size_t)S * 4), i_off = in.put((size_t)S * 8), i_bases = in.put((size_t)(b->n_words + 1) * 4);
    sl.cons_cap = r->cons_off[W];
    sl.solid_cap = want_solid ? r->solid_off[W] : 0;
    const size_t o_cons = out.put(sl.cons_cap), o_coff = out.put((size_t)(W + 1) * 8);
    sl.o_clen = out.put((size_t)W * 4); sl.o_stat = out.put(W);
    const size_t o_solid = out.put(sl.solid_cap * 4), o_soff = out.put((size_t)(W + 1) * 8);
    sl.o_slen = out.put((size_t)W * 4);
    sl.o_pc = out.put(sl.cons_cap); sl.o_ps = out.put(sl.solid_cap * 4); /* the compacted copies */
    const size_t o_pco = out.put((size_t)(W + 1) * 8), o_pso = out.put((size_t)(W + 1) * 8);
    sl.o_tot = out.put(48);
    sl.o_cons = o_cons; sl.o_solid = o_solid;
    int rc = ensure(&sl.dev_in, &sl.dev_in_bytes, in.bytes);
    if (rc) return rc;
    rc = ensure(&sl.dev_out, &sl.dev_out_bytes, out.bytes);
    if (rc) return rc;
    uint8_t* din = (uint8_t*)sl.dev_in;
    uint8_t* dout = (uint8_t*)sl.dev_out;
    hipStream_t ci = e->copy_in;
    CW_HIP(hipMemcpyAsync(din + i_wfs, b->win_first_seq, (size_t)(W + 1) * 4, hipMemcpyHostToDevice, ci));
    CW_HIP(hipMemcpyAsync(din + i_len, b->seq_len, (size_t)S * 4, hipMemcpyHostToDevice, ci));
    CW_HIP(hipMemcpyAsync(din + i_off, b->seq_word_off, (size_t)S * 8, hipMemcpyHostToDevice, ci));
    CW_HIP(hipMemcpyAsync(din + i_bases, b->bases, (size_t)b->n_words * 4, hipMemcpyHostToDevice, ci));
    CW_HIP(hipMemsetAsync(din + i_bases + (size_t)b->n_words * 4, 0, 4, ci));
    CW_HIP(hipMemcpyAsync(dout + o_coff, r->cons_off, (size_t)(W + 1) * 8, hipMemcpyHostToDevice, ci));
    if (want_solid) CW_HIP(hipMemcpyAsync(dout + o_soff, r->solid_off, (size_t)(W + 1) * 8, hipMemcpyHostToDevice, ci));
    CW_HIP(hipEventRecord(sl.ev_in, ci));
    hipStream_t st = e->stream;
    CW_HIP(hipStreamWaitEvent(st, sl.ev_in, 0));

    cw_batch db = *b;
    db.win_first_seq = (const uint32_t*)(din + i_wfs); db.seq_len = (const uint32_t*)(din + i_len);
    db.seq_word_off = (const uint64_t*)(din + i_off); db.bases = (const uint32_t*)(din + i_bases);
    cw_result dr;
    dr.cons = (char*)(dout + o_cons); dr.cons_off = (const uint64_t*)(dout + o_coff); dr.cons_len = (uint32_t*)(dout + sl.o_clen);
    dr.win_status = dout + sl.o_stat;
    dr.solid = want_solid ? (uint32_t*)(dout + o_solid) : nullptr;
    dr.solid_off = want_solid ? (const uint64_t*)(dout + o_soff) : nullptr;
    dr.solid_len = want_solid ? (uint32_t*)(dout + sl.o_slen) : nullptr;
    rc = run_device_locked(e, &db, &dr, st, pf_full);
    if (rc) return rc;
    PackArgs pa;
    pa.n_windows = W; pa.cons = dr.cons; pa.cons_off = dr.cons_off; pa.cons_len = dr.cons_len; pa.win_status = dr.win_status;
    pa.solid = dr.solid; pa.solid_off = dr.solid_off; pa.solid_len = dr.solid_len;
    pa.pc = (char*)(dout + sl.o_pc); pa.ps = (uint32_t*)(dout + sl.o_ps);
    pa.pc_off = (uint64_t*)(dout + o_pco); pa.ps_off = (uint64_t*)(dout + o_pso); pa.totals = (uint64_t*)(dout + sl.o_tot);
    pa.win = (const WinInfo*)e->scratch; /* this batch's: the pack kernels follow its finish kernel on the compute stream */
    pa.used = (const uint32_t*)((const uint8_t*)e->scratch + e->last_ctr_off + offsetof(BatchCounters, n_tasks));
    pa.pf_full_elems = (uint64_t)e->tmax_plan * kPfRowsMax;
    static_assert(offsetof(BatchCounters, n_members) == offsetof(BatchCounters, n_tasks) + 4, "cw_pack_scan_kernel reads the two counters as a pair");
    cw_pack_scan_kernel<<<1, 1024, 0, st>>>(pa);
    cw_pack_copy_kernel<<<(W + 3) / 4, 256, 0, st>>>(pa);
    CW_HIP(hipGetLastError());
    CW_HIP(hipEventRecord(sl.ev_done, st));
    sl.busy = true; sl.waiting = false;
    *ticket = si;
    return CW_OK;
}

int cw_submit(cw_engine* e, const cw_batch* b, const cw_result* r, int* ticket) { return submit_locked(e, b, r, ticket, false); }

/* why_tasks (may be NULL): how many windows of THIS ticket stopped on the batch's task / member / arena capacities; why_matrix: on the matrix slot */
/* used (may be NULL): this ticket's task and member counts */
static int wait_ticket(cw_engine* e, int ticket, uint64_t* why_tasks, uint32_t* used = nullptr, uint32_t* why_matrix = nullptr) {
    if (why_tasks) *why_tasks = 0;
    if (why_matrix) *why_matrix = 0;
    if (used) used[0] = used[1] = 0xFFFFFFFFu;
    if (!e || ticket < 0 || ticket >= CW_SLOTS) return CW_E_INVALID;
    cw_slot& sl = e->slot[ticket];
    {
        std::lock_guard<std::mutex> lk(e->mu);
        if (!sl.busy || sl.waiting) return CW_E_INVALID; /* a ticket is waited for once: a second waiter would race on the staging buffers */
        if (sl.n_windows == 0) { sl.busy = false; return CW_OK; }
        sl.waiting = true;
    }
    /* the slot belongs to this ticket until busy is cleared; other threads may submit meanwhile */
    auto fail = [&](int code) { std::lock_guard<std::mutex> lk(e->mu); sl.busy = false; sl.waiting = false; return code; };
    if (hipSetDevice(e->device) != hipSuccess || hipEventSynchronize(sl.ev_done) != hipSuccess) return fail(CW_E_NO_DEVICE);
    const uint32_t W = sl.n_windows;
    const cw_result& r = sl.res;
    uint8_t* dout = (uint8_t*)sl.dev_out;
    hipStream_t co = e->copy_out;
    uint64_t tot[6] = {0, 0, 0, 0, 0, 0};
    int rc = CW_OK;
    if (hipMemcpyAsync(tot, dout + sl.o_tot, 48, hipMemcpyDeviceToHost, co) != hipSuccess ||
        hipMemcpyAsync(r.cons_len, dout + sl.o_clen, (size_t)W * 4, hipMemcpyDeviceToHost, co) != hipSuccess ||
        hipMemcpyAsync(r.win_status, dout + sl.o_stat, W, hipMemcpyDeviceToHost, co) != hipSuccess ||
        (sl.want_solid && hipMemcpyAsync(r.solid_len, dout + sl.o_slen, (size_t)W * 4, hipMemcpyDeviceToHost, co) != hipSuccess) ||
        hipStreamSynchronize(co) != hipSuccess)
        return fail(CW_E_NO_DEVICE);
    if (tot[0] > sl.cons_cap || tot[1] > sl.solid_cap) return fail(CW_E_INTERNAL);
    if (why_tasks) *why_tasks = tot[2];
    if (why_matrix) *why_matrix = (uint32_t)tot[5];
    if (used) { used[0] = (uint32_t)tot[3]; used[1] = (uint32_t)tot[4]; }
    const size_t need = align_up(tot[0], 256) + tot[1] * 4 + 256;
    if (sl.pin_out_bytes < need) {
        if (sl.pin_out) (void)hipHostFree(sl.pin_out);
        sl.pin_out = nullptr; sl.pin_out_bytes = 0;
        const size_t want = need + need / 4; /* some slack: the next batch is rarely exactly as large */
        if (hipHostMalloc(&sl.pin_out, want, hipHostMallocDefault) != hipSuccess) { sl.pin_out = nullptr; return fail(CW_E_NOMEM); }
        sl.pin_out_bytes = want;
    }
    char* hc = (char*)sl.pin_out;
    uint32_t* hs = (uint32_t*)((uint8_t*)sl.pin_out + align_up(tot[0], 256));
    if ((tot[0] && hipMemcpyAsync(hc, dout + sl.o_pc, tot[0], hipMemcpyDeviceToHost, co) != hipSuccess) ||
        (tot[1] && hipMemcpyAsync(hs, dout + sl.o_ps, tot[1] * 4, hipMemcpyDeviceToHost, co) != hipSuccess) ||
        hipStreamSynchronize(co) != hipSuccess)
        return fail(CW_E_NO_DEVICE);
    uint64_t pc = 0, ps = 0;
    for (uint32_t w = 0; w < W; ++w) {
        const bool ok = r.win_status[w] != CW_WIN_OVERFLOW;
        if (!ok) rc = CW_E_CAPACITY;
        const uint32_t cl = ok ? r.cons_len[w] : 0u;
        if (cl) memcpy(r.cons + r.cons_off[w], hc + pc, cl);
        pc += cl;
        if (sl.want_solid) {
            const uint32_t n = ok ? r.solid_len[w] : 0u;
            if (n) memcpy(r.solid + r.solid_off[w], hs + ps, (size_t)n * 4);
            ps += n;
        }
    }
    if (pc != tot[0] || ps != tot[1]) rc = CW_E_INTERNAL;
    return fail(rc);
}

int cw_wait(cw_engine* e, int ticket) { return wait_ticket(e, ticket, nullptr); }

/* After a finished run: did windows stop on a capacity that a larger scratch plan cures (CW_WHY_TASKS: the task, member and arena slots are
   heuristics of the batch)?  Then the plan grows (x4, up to x64) and the caller runs the batch again -- if the larger plan is one the engine can
   actually run: inside the 32-bit offsets (plan_scratch clamps the arena's own scale) and inside the device's free memory.  A scale that is not
   is refused here, and the run that has finished stands with its overflow statuses (it used to end the batch with CW_E_INVALID or
   CW_E_NOMEM).  Windows stopped on the index kernel's global matrix slot (CW_WHY_MATRIX: sized from the batch's mean depth) have the batch run
   again with that slot at its full kPfRowsMax rows (*pf_full, for the re-run only: the scale stays) -- unless each of them needs more than that
   (the index kernel leaves the need in WinInfo::arena_used): a pile too deep for any slot does not make the batch run twice.  known_any: -1 = look at the last run's
   WinInfo in scratch (cw_run_device_sync: the caller has just waited for that very run); 0..7 = the caller knows from its own ticket which kinds
   of such windows exist (bit 0 task / member slots, bit 1 arena slices, bit 2 the matrix slot) (cw_run: scratch may already belong to another
   thread's batch). */
static int grow_if_that_helps(cw_engine* e, bool* again, bool* pf_full, hipStream_t st, int known_any, uint32_t n_windows, uint32_t n_seqs, uint64_t n_words) {
    *again = false;
    std::lock_guard<std::mutex> lk(e->mu);
    if (!e->scratch || n_windows == 0) return CW_OK;
    CW_HIP(hipSetDevice(e->device));
    int kinds = known_any > 0 ? known_any : 0; /* bit 0: windows stopped on task / member slots, bit 1: on their arena slices, bit 2: on the matrix slot */
    if (known_any < 0) {
        if (e->last_windows != n_windows) return CW_OK;
        if (int rc = read_counters(e, st, offsetof(BatchCounters, any_overflow), 4, &e->host_fb->any_overflow)) return rc;
        if (!e->host_fb->any_overflow) return CW_OK;
        std::vector<WinInfo> wi(e->last_windows);
        CW_HIP(hipMemcpyAsync(wi.data(), e->scratch, (size_t)e->last_windows * sizeof(WinInfo), hipMemcpyDeviceToHost, st));
        CW_HIP(hipStreamSynchronize(st));
        /* (windows stopped for other reasons stay stopped: the loop ends when no window names these capacities, or at x64) */
        for (const WinInfo& w : wi)
            if (w.status == CW_WIN_OVERFLOW)
                kinds |= w.pad_ == CW_WHY_TASKS ? 1 : w.pad_ == CW_WHY_ARENA ? 2 : w.pad_ == CW_WHY_MATRIX && w.arena_used <= (uint64_t)e->tmax_plan * kPfRowsMax ? 4 : 0;
    }
    if (CW_AID_ENV("CW_TASK_CAP") || CW_AID_ENV("CW_MEMBER_CAP")) kinds &= 4; /* (test aids that shrink exactly the task / member capacities) */
    if (!kinds) return CW_OK;
    PlanInput in = plan_input(e, n_windows, n_seqs, n_words), in_up = in;
    in.pf_full = in_up.pf_full = *pf_full; in_up.scale = e->cap_scale * 4u;
    const ScratchPlan cur = plan_scratch(in);
    const bool pf_grows = (kinds & 4) && cur.pfall_elems < (uint64_t)e->tmax_plan * kPfRowsMax;
    uint32_t next = e->cap_scale;
    if ((kinds & 3) && e->cap_scale < 64u) {
        /* does the larger plan grow what ran out?  (the arena's own scale is clamped to 32-bit offsets: a batch stopped on its arena slices
           at a clamped scale is the same batch with the same arena at x4, x16 and x64) */
        const ScratchPlan up = plan_scratch(in_up);
        if (((kinds & 1) && (up.task_cap > cur.task_cap || up.member_cap > cur.member_cap)) || ((kinds & 2) && up.arena_scale > cur.arena_scale)) next = e->cap_scale * 4u;
        else fprintf(stderr, "[consent_amd] windows stopped on the batch's %s capacity; a plan x%u does not enlarge it: keeping the run's result\n", (kinds & 2) ? "arena" : "task / member", e->cap_scale * 4u);
    }
    if (next == e->cap_scale && !pf_grows) return CW_OK;
    in.scale = next; in.pf_full = *pf_full || pf_grows;
    const ScratchPlan p = plan_scratch(in);
    size_t free_b = 0, total_b = 0;
    const bool mem_known = hipMemGetInfo(&free_b, &total_b) == hipSuccess;
    if (!mem_known) (void)hipGetLastError();
    const size_t margin = (size_t)2 << 30; /* other engines of the device grow too */
    const bool fits = p.solid_cap <= 0xFFFFFFFFull && p.seg_cap <= 0xFFFFFFFFull && p.arena_cap <= 0xFFFFFFFFull &&
                      (!mem_known || p.total <= e->scratch_bytes || p.total - e->scratch_bytes + margin <= free_b);
    if (!fits) {
        fprintf(stderr, "[consent_amd] windows stopped on the batch's task / member / arena / matrix capacities; a plan x%u (%.1f GB) does not fit this device now: keeping the run's result\n",
                next, (double)p.total / 1e9);
        return CW_OK;
    }
    if (pf_grows) *pf_full = true;
    if (next != e->cap_scale) {
        e->cap_scale = next;
        fprintf(stderr, "[consent_amd] windows stopped on the batch's task / member / arena capacities: running the batch again with the plan x%u\n", e->cap_scale);
    }
    *again = true;
    return CW_OK;
}

/* A grown plan is not forever: after a run at scale > 1 that used less than half of what the next smaller plan offers, the
   scale goes back a step; scratch that has become three times what the smaller plan needs is given back to the device. */
/* known (may be NULL): the run's own task and member counts (cw_run: its ticket's totals -- the counters in scratch may by now be another thread's batch);
   NULL: read them from scratch (cw_run_device_sync: the caller has just waited for that very run).  Scratch is only given back when nothing of this
   engine is in flight. */
static void decay_scale(cw_engine* e, hipStream_t st, uint32_t n_windows, uint32_t n_seqs, uint64_t n_words, const uint32_t* known = nullptr) {
    std::lock_guard<std::mutex> lk(e->mu);
    if (e->cap_scale <= 1u || !e->scratch || (!known && e->last_windows != n_windows)) return;
    if (hipSetDevice(e->device) != hipSuccess) return;
    uint32_t* used = e->host_fb->used; /* n_tasks, n_members */
    if (known) { if (known[0] == 0xFFFFFFFFu) return; used[0] = known[0]; used[1] = known[1]; }
    else if (read_counters(e, st, offsetof(BatchCounters, n_tasks), 8, used) != CW_OK) { (void)hipGetLastError(); return; }
    PlanInput in = plan_input(e, n_windows, n_seqs, n_words); in.scale = e->cap_scale / 4u;
    const ScratchPlan lower = plan_scratch(in);
    if ((uint64_t)used[0] * 2u > lower.task_cap || (uint64_t)used[1] * 2u > lower.member_cap) return;
    e->cap_scale /= 4u;
    bool in_flight = false;
    for (int i = 0; i < CW_SLOTS; ++i) in_flight = in_flight || e->slot[i].busy; /* (cw_run: another thread's batch may be running on this scratch) */
    if (!in_flight && e->scratch_bytes > 3 * lower.total + ((size_t)1 << 30)) { /* nothing of this engine is in flight: the caller has just waited for its stream */
        if (hipFree(e->scratch) != hipSuccess) (void)hipGetLastError();
        e->scratch = nullptr; e->scratch_bytes = 0;
    }
}

/* One finished attempt at a batch.  launch_rc not CW_OK: it could not be set up and none of its kernels was launched.  rc, of the finished run: CW_OK, CW_E_CAPACITY
   (windows stopped: the result stands), or an error that ends the loop.  known_any, used: grow_if_that_helps' and decay_scale's `known`.  st: the stream the two read scratch with. */
struct Attempt { int launch_rc, rc, known_any; const uint32_t* used; hipStream_t st; };

/* Run a batch, and -- when windows stopped on the batch's task / member / arena / matrix capacities only -- once more with a larger plan, up to x64
   (grow_if_that_helps); after a run that needed no growth, see whether a grown scale can go back (decay_scale).  attempt(pf_full) launches one run and waits for it.
   A re-run whose larger plan could not be set up after all (memory went to another engine meanwhile) launched nothing: the run before it stands and the scale goes back. */
extern "C++" { /* (a template cannot have C linkage) */
template <class F>
static int run_and_regrow(cw_engine* e, uint32_t n_windows, uint32_t n_seqs, uint64_t n_words, F attempt) {
    bool grown = false, pf_full = false;
    uint32_t scale_before = 1;
    int first_rc = CW_OK;
    for (;;) {
        const Attempt a = attempt(pf_full);
        if (a.launch_rc != CW_OK) {
            if (!grown || (a.launch_rc != CW_E_INVALID && a.launch_rc != CW_E_NOMEM)) return a.launch_rc;
            std::lock_guard<std::mutex> lk(e->mu);
            e->cap_scale = scale_before;
            return first_rc;
        }
        if (a.rc != CW_OK && a.rc != CW_E_CAPACITY) return a.rc;
        bool again = false;
        { std::lock_guard<std::mutex> lk(e->mu); scale_before = e->cap_scale; }
        if (a.known_any < 0 || a.rc == CW_E_CAPACITY)
            if (const int rc = grow_if_that_helps(e, &again, &pf_full, a.st, a.known_any, n_windows, n_seqs, n_words)) return rc;
        if (!again) {
            if (!grown && a.rc == CW_OK) decay_scale(e, a.st, n_windows, n_seqs, n_words, a.used); /* the host path never lowered a grown scale */
            return a.rc;
        }
        grown = true; first_rc = a.rc;
    }
}
} // extern "C++"

/* cw_run_device, then wait for the stream, then -- when windows stopped on the batch's task / member / arena capacities only -- once more
   with a larger plan (cw_private.h; what the native driver calls: the asynchronous cw_run_device cannot look at its own result; the statuses stay on the device) */
int cw_run_device_sync(cw_engine* e, const cw_batch* batch, const cw_result* res, void* hip_stream) {
    if (!e || !batch) return CW_E_INVALID;
    return run_and_regrow(e, batch->n_windows, batch->n_seqs, batch->n_words, [&](bool pf_full) {
        int lrc;
        { std::lock_guard<std::mutex> lk(e->mu); lrc = run_device_locked(e, batch, res, hip_stream, pf_full); }
        hipStream_t st = hip_stream ? (hipStream_t)hip_stream : e->stream;
        const bool waited = lrc != CW_OK || (hipSetDevice(e->device) == hipSuccess && hipStreamSynchronize(st) == hipSuccess);
        return Attempt{lrc, waited ? CW_OK : CW_E_NO_DEVICE, -1, nullptr, st};
    });
}

/* cw_submit + cw_wait in the same loop.  The decision comes from this ticket's own totals (cw_pack_scan_kernel counts the windows stopped on CW_WHY_TASKS /
   _ARENA / _MATRIX and the tasks and members used): other threads may have submitted since, and the WinInfo in scratch may be theirs */
int cw_run(cw_engine* e, const cw_batch* b, const cw_result* r) {
    if (!e || !b) return CW_E_INVALID;
    uint32_t used[2];
    return run_and_regrow(e, b->n_windows, b->n_seqs, b->n_words, [&](bool pf_full) {
        int t = -1;
        uint64_t why_tasks = 0;
        uint32_t why_matrix = 0;
        const int lrc = submit_locked(e, b, r, &t, pf_full);
        const int rc = lrc == CW_OK ? wait_ticket(e, t, &why_tasks, used, &why_matrix) : CW_OK;
        return Attempt{lrc, rc, ((uint32_t)why_tasks ? 1 : 0) | ((why_tasks >> 32) ? 2 : 0) | (why_matrix ? 4 : 0), used, e->stream};
    });
}

/* pinned host memory for batches and results: copies from and to it are real DMA transfers that overlap the kernels; plain
   (pageable) buffers work too, but the runtime stages them through its own bounce buffers and the overlap is lost */
int cw_host_alloc(void** ptr, size_t bytes) {
    if (!ptr) return CW_E_INVALID;
    *ptr = nullptr;
    if (hipHostMalloc(ptr, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) { *ptr = nullptr; return CW_E_NOMEM; }
    return CW_OK;
}

void cw_host_free(void* ptr) {
    if (ptr) (void)hipHostFree(ptr);
}

} // extern "C"
