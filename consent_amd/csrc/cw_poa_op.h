/*
 * cw_poa_op.h -- the POA tiers as a batched consensus operator (cw_poa_run / cw_poa_run_device, include/consent_amd.h): a front and a back around the POA
 * stage of a window run (cw_engine.cpp enqueue_poa_stage), which is unchanged.
 *
 *   cw_poa_tasks_kernel   stands where setup + index + chain stand: one POA task per GROUP of the batch (task index = group index), its members the group's
 *                         first max_msa non-empty sequences in the order given, routed by the chain kernel's rule (cw_poa_route, cw_poa_q.h); what the POA stage
 *                         expects from cw_setup_kernel (WinInfo status, the neutral task, seg_off / seg_len) comes from here too.
 *   cw_poa_gather_kernel  stands where cw_finish_kernel stands: per group the status, cons_len and the consensus, copied from the arena to the caller's slot.
 *
 * A group is "window" g of the batch and owns segment slot g; its arena slot is what the chain kernel reserves for a segment (CW_POA_SLOT_BYTES of the
 * longest member, or the one member's length), bumped from BatchCounters::poa_arena_used.  The plan of such a run is cw_plan.h plan_poa.
 */
#ifndef CW_POA_OP_H
#define CW_POA_OP_H

#include "cw_device.h"
#include "cw_poa.h"   /* CW_POAX_LC */
#include "cw_poa_q.h" /* cw_poa_route */

#define CW_POAOP_WAVES 4 /* groups per work-group of the two kernels: one wave each */

/* where a run's consensuses go: cw_result without the solid fields */
struct PoaOut {
    char* cons;
    const uint64_t* cons_off;
    uint32_t* cons_len;
    uint8_t* win_status;
};

/* One wave per group, lanes over its sequences in rounds of 64.  The group's member range in members[] is its own sequence range (a group has no more members
   than sequences), so only the arena slot and the tier-list entry need an atomic: one each per wave. */
__global__ void __launch_bounds__(64 * CW_POAOP_WAVES) cw_poa_tasks_kernel(DevBatch b, DevScratch sc, uint32_t max_msa, uint32_t n_seqs, uint64_t arena_cap) {
    const int lane = threadIdx.x & 63;
    const uint32_t g = blockIdx.x * CW_POAOP_WAVES + (threadIdx.x >> 6);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        /* the neutral task (cw_setup_kernel's): what a list entry beyond a capacity would name -- none here, the lists hold a task per group -- and the batch's totals */
        PoaTask t; t.window = 0; t.seg_slot = 0; t.member_off = 0; t.n_members = 0; t.max_len = 0; t.out_off = 0; t.out_cap = 0; t.state = 1u;
        sc.tasks[sc.task_cap] = t;
        sc.ctr->n_tasks = b.n_windows; /* task index = group index: tier S walks all of them and takes those in state 0 */
        sc.ctr->n_members = n_seqs;
    }
    if (g >= b.n_windows) return;
    const uint32_t s0 = b.win_first_seq[g], s1 = b.win_first_seq[g + 1];
    const unsigned long long below = (1ull << lane) - 1ull;
    uint32_t cnt = 0, mx = 0, sum = 0, first_seq = 0;
    bool too_long = false;
    for (uint32_t sb = s0; sb < s1 && cnt < max_msa; sb += 64) {
        const uint32_t s = sb + (uint32_t)lane;
        const uint32_t l = s < s1 ? b.seq_len[s] : 0u;
        const unsigned long long bal = __ballot(l > 0u);
        const uint32_t idx = cnt + (uint32_t)__popcll(bal & below);
        if (l > 0u && idx < max_msa) { /* zero-length sequences are skipped; the first max_msa others are aligned */
            too_long = too_long || l > (uint32_t)CW_POAX_LC;
            PoaMember pm;
            pm.seq = s; pm.start = 0; pm.len = (uint16_t)(l > 0xFFFFu ? 0xFFFFu : l); /* (a group with a member beyond tier X's bases gets no task: the field never wraps in one) */
            sc.members[s0 + idx] = pm;
            mx = max(mx, l); sum += l > 0xFFFFu ? 0xFFFFu : l;
        }
        if (cnt == 0 && bal != 0ull) first_seq = sb + (uint32_t)__builtin_ctzll(bal);
        cnt += (uint32_t)__popcll(bal);
    }
    const uint32_t n = cnt < max_msa ? cnt : max_msa;
    mx = (uint32_t)cw_wave_max((int)mx); sum = (uint32_t)cw_wave_sum((int)sum); /* (max_msa members of <= 65 535 bases: the sum fits while max_msa < 32 768; beyond that only the sort's order could differ) */
    const bool stop = __ballot(too_long) != 0ull;
    const bool poa = !stop && n > 1u;
    const uint32_t tier = cw_poa_route(sc, poa, n, mx);
    /* the group's arena slot: what the chain kernel reserves for a segment (cw_chain.h "need"), in units of 16 bytes so that the gather kernel reads it wide */
    const uint32_t need = stop || n == 0u ? 0u : n == 1u ? mx : 2u * mx + 2u;
    uint32_t off = 0, li = 0;
    if (lane == 0) {
        if (need) off = atomicAdd(&sc.ctr->poa_arena_used, (need + 15u) & ~15u);
        if (tier != 0xFFu && tier != 0u) li = atomicAdd(&sc.ctr->n_tier[tier == 4u ? 0 : tier], 1u);
    }
    off = (uint32_t)cw_lane_value((int)off, 0); li = (uint32_t)cw_lane_value((int)li, 0);
    const bool fits = (uint64_t)off + need <= arena_cap && li < sc.list_cap; /* (always: plan_poa's arena holds every group's slot, a list a task per group) */
    if (n == 1u && !stop && fits) { /* one member: the consensus is that member, straight into the slot (the flush's g_n == 1 branch) */
        const uint32_t* words = b.bases + b.seq_word_off[first_seq];
        for (uint32_t i = lane; i < mx; i += 64) sc.arena[off + i] = CW_ACGT(cw_base_at(words, i));
    }
    if (lane == 0) {
        WinInfo wi;
        wi.status = CW_WIN_CONSENSUS; wi.n_seqs = s1 - s0; wi.tpl_len = mx; wi.n_kmers = 0;
        wi.solid_base = 0; wi.solid_cap = 0; wi.n_solid = 0;
        wi.seg_base = g; wi.seg_cap = 1; wi.n_segs = 1;
        wi.arena_base = off; wi.arena_cap = need; wi.arena_used = 0;
        wi.ab_base = 0; wi.ab_cap = 0; wi.pad_ = 0;
        if (stop || !fits) { wi.status = CW_WIN_OVERFLOW; wi.pad_ = stop ? CW_WHY_POA : CW_WHY_ARENA; wi.n_segs = 0; sc.ctr->any_overflow = 1; }
        sc.win[g] = wi;
        PoaTask t;
        t.window = g; t.seg_slot = g; t.member_off = s0; t.out_off = off; t.out_cap = need;
        if (poa && fits) {
            t.n_members = n; t.max_len = mx | ((sum / n) << 16); /* longest member | mean member length: what the tier sort goes by (cw_chain.h) */
            t.state = tier ? 2u : 0u; /* 0 = tier S takes it from the task array; anything else is on a list */
            if (tier) sc.tier_list[tier == 4u ? 0 : tier][li] = cw_list_entry(sc, g, t.n_members, t.max_len, tier == 4u ? 0 : (int)tier); /* with its sort class, as the chain kernel's flush emits it */
        } else { /* nothing to align: a finished task without members */
            t.n_members = 0; t.max_len = 0; t.state = 1u;
            if (tier != 0xFFu && tier != 0u && li < sc.list_cap) sc.tier_list[tier == 4u ? 0 : tier][li] = cw_list_entry(sc, sc.task_cap, 0u, 0u, tier == 4u ? 0 : (int)tier);
        }
        sc.tasks[g] = t;
        sc.seg_off[g] = off; sc.seg_len[g] = (n == 1u && !stop && fits) ? mx : 0u;
    }
}

/* One wave per group: status (a stop recorded in WinInfo, a task that did not end as done, a consensus longer than the caller's slot), cons_len, and the
   consensus from the group's arena slot -- 16-byte aligned: plan_poa -- to the caller's: 16 bytes a lane where the caller's slot is aligned too. */
__global__ void __launch_bounds__(64 * CW_POAOP_WAVES) cw_poa_gather_kernel(DevBatch b, DevScratch sc, PoaOut out) {
    const int lane = threadIdx.x & 63;
    const uint32_t g = blockIdx.x * CW_POAOP_WAVES + (threadIdx.x >> 6);
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicMax(sc.step_clock, (unsigned long long)wall_clock64()); /* when this batch ended (cw_finish_kernel does the same) */
    if (g >= b.n_windows) return;
    const uint32_t w_status = sc.win[g].status, t_state = sc.tasks[g].state, len = sc.seg_len[g], off = sc.seg_off[g];
    const uint64_t o0 = out.cons_off[g], o1 = out.cons_off[g + 1];
    const uint64_t slot = o1 > o0 ? o1 - o0 : 0;
    uint32_t why = 0;
    if (w_status == CW_WIN_OVERFLOW) why = sc.win[g].pad_ ? sc.win[g].pad_ : CW_WHY_POA;
    else if (t_state != 1u) why = CW_WHY_POA; /* (a task no tier finished: every such task has stopped its group already) */
    else if (len > slot) why = CW_WHY_OUT_CONS; /* never a truncation */
    if (why) {
        if (lane == 0) {
            sc.win[g].status = CW_WIN_OVERFLOW; sc.win[g].pad_ = why; sc.ctr->any_overflow = 1;
            out.cons_len[g] = 0; out.win_status[g] = CW_WIN_OVERFLOW;
        }
        return;
    }
    const uint8_t* src = sc.arena + off;
    char* dst = out.cons + o0;
    const uint32_t wide = (((uintptr_t)dst | (uintptr_t)src) & 15u) == 0u ? len & ~15u : 0u;
    for (uint32_t i = (uint32_t)lane * 16u; i < wide; i += 64u * 16u) *(uint4*)(dst + i) = *(const uint4*)(src + i);
    for (uint32_t i = wide + (uint32_t)lane; i < len; i += 64u) dst[i] = (char)src[i];
    if (lane == 0) { out.cons_len[g] = len; out.win_status[g] = CW_WIN_CONSENSUS; }
}

#endif
