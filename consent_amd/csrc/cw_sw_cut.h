/*
 * cw_sw_cut.h -- the alignment operator's cut run (cw_sw_cut_run / cw_sw_cut_run_device, include/consent_amd.h): per pair the row of cw_sw_path_run, and
 * instead of the path's ops where the query crosses the reference's window boundaries: word t of a query's slot is the query position at reference column
 * t x W, so that piece t of the query is what its alignment puts on window t.  And cw_cut_groups_device on top of it: the POA batch of every (reference, window)
 * -- the window's columns first, then piece t of every query whose alignment spans the window.  The cut kernels are calls of cw_sw_op.h's sw_class_loop / sw_long_loop (LDS slabs,
 * per-wave scratch, pair-claim loop, under the launch bounds of the path kernels) around cut_pair, which follows sw_path_pair line by line up to the closed walk.
 * The run's own are:
 *
 *   cw_sw_cut_rest_kernel   one thread per sequence, behind the order kernel: a query whose row the order kernel wrote (beyond a capacity, empty, or on an empty
 *                           reference) never reaches a wave; its T + 1 zeros are stored here, where its slot holds them.
 *   cut_mark                wave-wide, where pile_count stands: the walk's steps in alignment order, 64 a round, (i, j) of a step the prefix sums of what the
 *                           steps before it consumed.  A lane whose step consumes a column (M or D) that is a multiple of W beyond ref_begin stores the query
 *                           position to that window's word; then the lanes fill the words of the boundaries at or before ref_begin with query_begin and those
 *                           beyond ref_end with query_end + 1.  A path consumes a column once, and the three sets of boundaries are disjoint: every word is
 *                           stored once, with a plain store.  Nothing depends on wave order, so the words depend on no batch composition.
 *   cw_cut_count_kernel     one wave per (reference, window), lanes over the group's queries in rounds of 64: members and packed words of the output group.
 *   cw_cut_scan_kernel      exclusive prefix sums over the output groups (cw_extract_scan_kernel's).
 *   cw_cut_fill_kernel      one wave per output group again: the member index by ballot prefix, every member's words assembled a 16-base word a lane and step.
 */
#ifndef CW_SW_CUT_H
#define CW_SW_CUT_H

#include "cw_sw_path.h"

struct CutArgs {
    SwArgs a;                /* as for cw_sw_path_run: a.dir / a.dir_bytes are CW_SW_PATH_BYTES per wave */
    uint32_t* cuts;          /* the caller's */
    const uint64_t* cut_off; /* [n_seqs + 1] */
    uint32_t window;         /* W >= 1 */
    uint8_t* steps;          /* CW_SW_STEP_BYTES per wave of the largest grid */
};

/* the windows of a reference of n columns */
__device__ __forceinline__ uint32_t cut_windows(uint32_t n, uint32_t W) { return n / W + (n % W != 0u ? 1u : 0u); }

/* whether sequence s's slot holds the T + 1 words of a query on a reference of T windows */
__device__ __forceinline__ bool cut_slot_holds(const uint64_t* cut_off, uint32_t s, uint32_t T) {
    const uint64_t o0 = cut_off[s], o1 = cut_off[s + 1];
    return o1 >= o0 && o1 - o0 >= (uint64_t)T + 1u;
}

/* phase 0 of the order kernel wrote the rows of the sequences that are no pair (seq_ref = none): of those every one but a reference is a query that does not
   count */
__global__ void __launch_bounds__(256) cw_sw_cut_rest_kernel(CutArgs ca) {
    const SwArgs& a = ca.a;
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    if (s >= a.n_seqs || a.seq_ref[s] != 0xFFFFFFFFu) return;
    uint32_t lo = 0, hi = a.b.n_windows; /* the group of s, as the order kernel finds it */
    while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (a.b.win_first_seq[mid] <= s) lo = mid; else hi = mid; }
    const uint32_t r = a.b.win_first_seq[lo];
    if (s == r) return;
    const uint32_t T = cut_windows(a.b.seq_len[r], ca.window);
    if (!cut_slot_holds(ca.cut_off, s, T)) return;
    uint32_t* const slot = ca.cuts + ca.cut_off[s];
    for (uint32_t t = 0; t <= T; ++t) slot[t] = 0u;
}

/* a pair that does not count: T + 1 zeros */
__device__ __forceinline__ void cut_zero(uint32_t* slot, uint32_t T, int lane) {
    for (uint32_t t = (uint32_t)lane; t <= T; t += 64u) slot[t] = 0u;
}

/* the cut points of n steps of a closed path from (qb, rb) to (qe, re), all absolute, on a reference of T windows of W columns; slot: the query's T + 1 words */
__device__ __forceinline__ void cut_mark(const uint8_t* steps, uint32_t n, uint32_t rb, uint32_t re, uint32_t qb, uint32_t qe, uint32_t W, uint32_t T, uint32_t* slot, int lane) {
    uint32_t ci = 0, cj = 0;
    for (uint32_t base = 0; base < n; base += 64u) {
        const uint32_t k = base + (uint32_t)lane;
        const bool on = k < n;
        const int c = on ? (int)steps[n - 1u - k] : 3;
        const int di = on && c != 2 ? 1 : 0, dj = on && c != 1 ? 1 : 0;
        const int si = cw_wave_scan_add(di), sj = cw_wave_scan_add(dj);
        const uint32_t i0 = ci + (uint32_t)(si - di), j0 = cj + (uint32_t)(sj - dj);
        const uint32_t col = rb + j0;
        if (on && c != 1 && j0 > 0u && col <= re && col % W == 0u) slot[col / W] = qb + i0; /* (col <= re < n: the word is below T) */
        ci += (uint32_t)cw_lane_value(si, 63); cj += (uint32_t)cw_lane_value(sj, 63);
    }
    for (uint32_t t = (uint32_t)lane; t <= rb / W; t += 64u) slot[t] = qb;            /* t x W <= ref_begin */
    for (uint32_t t = re / W + 1u + (uint32_t)lane; t <= T; t += 64u) slot[t] = qe + 1u; /* t x W > ref_end */
}

/* one pair on one wave, its buffers in place, as sw_path_pair: align, the banded pass, the walk -- then the cut points in place of the ops -- the row */
template <int CLS, bool SPAN>
__device__ __forceinline__ void cut_pair(const CutArgs& ca, uint32_t s, uint8_t* refc, uint8_t* qfw, uint8_t* qrv, uint32_t qrv_bytes, bool qrv_lds, uint8_t* rows, uint8_t* dirbuf, uint8_t* steps,
                                         uint8_t* state, int lane) {
    const SwArgs& a = ca.a;
    const uint32_t r = st_uni(a.seq_ref[s]);
    const uint32_t m = st_uni(a.b.seq_len[s]), n = st_uni(a.b.seq_len[r]);
    const uint32_t sn = sw_unpack_ref<SPAN>(a, refc, s, r, n, lane);
    sw_unpack(qfw, a.b.bases + a.b.seq_word_off[s], m, lane);
    st_mem_sync();
    const StAlign al = sw_align<CLS>(qfw, (int)m, qrv, refc, (int)sn, lane, state); /* in the span's coordinates, as everything up to the walk */
    uint32_t ins = 0, del = 0;
    int status = CW_SW_ALIGNED;
    const uint32_t T = cut_windows(n, ca.window);
    const bool holds = cut_slot_holds(ca.cut_off, s, T);
    uint32_t* const slot = ca.cuts + ca.cut_off[s];
    bool marked = false;
    if (al.score > 0) {
        const int refLen = st_uni(al.ref_end - al.ref_begin + 1), readLen = st_uni(al.query_end - al.query_begin + 1);
        const uint8_t* const ref0 = refc + al.ref_begin; const uint8_t* const read0 = qfw + al.query_begin;
        const SwBand bd = sw_banded_path(ref0, refLen, read0, readLen, st_uni(al.score), rows, dirbuf, a.dir_bytes, qrv_lds ? qrv : nullptr, qrv_lds ? qrv_bytes : 0u, lane);
        if (!bd.fits) status = CW_SW_NO_PATH;
        else {
            const SwWalk w = sw_walk(bd, refLen, readLen, steps, lane);
            ins = w.ins; del = w.del;
            if (!w.closed) status = CW_SW_PATH_OPEN;
            else {
                const SwSpan sl{st_uni(sw_pair_lo<SPAN>(a, s)), st_uni(sw_pair_len<SPAN>(a, s, n))};
                if (!holds || al.ref_begin < 0 || al.query_begin < 0 || (uint32_t)al.ref_begin + (uint32_t)refLen > sl.len) status = CW_SW_CUT_SLOT; /* (the ends lie inside the span, the span inside the reference) */
                else { /* the boundaries are the whole reference's: absolute ends */
                    cut_mark(steps, w.n_steps, sl.lo + (uint32_t)al.ref_begin, sl.lo + (uint32_t)al.ref_end, (uint32_t)al.query_begin, (uint32_t)al.query_end, ca.window, T, slot, lane);
                    marked = true;
                }
            }
        }
    }
    if (!marked && holds && status != CW_SW_CUT_SLOT) cut_zero(slot, T, lane); /* a pair that does not count */
    if (lane == 0) {
        const int lo = al.score > 0 ? (int)sw_pair_lo<SPAN>(a, s) : 0; /* the row is absolute */
        sw_write_row(a.rows + (size_t)s * CW_SW_ROW, al.score, al.ref_begin + lo, al.ref_end + lo, al.query_begin, al.query_end, ins, del, status);
    }
    st_mem_sync(); /* the next pair's unpacking overwrites what this one read */
}

template <int CLS, bool SPAN>
__global__ void __launch_bounds__(64 * CW_SW_WAVES, CLS == 0 ? 4 : 1) cw_sw_cut_kernel(CutArgs ca) {
    sw_class_loop<CLS, true, SPAN>(ca.a, ca.steps, [&](uint32_t s, const SwWaveBufs& w, int lane) __attribute__((always_inline)) {
        cut_pair<CLS, SPAN>(ca, s, w.refc, w.qfw, w.qrv, w.qrv_bytes, w.qrv_lds, w.rows, w.dirbuf, w.steps, w.state, lane);
    });
}

template <bool SPAN>
__global__ void __launch_bounds__(64, 2) cw_sw_cut_long_kernel(CutArgs ca) {
    sw_long_loop<true>(ca.a, ca.steps, [&](uint32_t s, const SwWaveBufs& w, int lane) __attribute__((always_inline)) {
        cut_pair<2, SPAN>(ca, s, w.refc, w.qfw, w.qrv, w.qrv_bytes, w.qrv_lds, w.rows, w.dirbuf, w.steps, w.state, lane);
    });
}

/* ---- cw_cut_groups_device: the POA batch of every (reference, window) --------------------------------------------------------------------------------------- */

struct CutGroupArgs {
    DevBatch b;              /* the groups of the cut run */
    const int32_t* rows;     /* its rows */
    const uint32_t* cuts;    /* its slots */
    const uint64_t* cut_off;
    uint32_t window;
    uint32_t out_cap;        /* output groups the working arrays hold */
    uint32_t* grp;           /* [n_windows + 1] working: windows per input group, then exclusive offsets; [n_windows] = output groups */
    uint32_t* win_seqs;      /* [out_cap + 1] counts, then exclusive offsets */
    uint64_t* win_words;     /* [out_cap + 1] */
    /* outputs */
    uint32_t* grp_first;
    uint32_t* win_first_seq;
    uint32_t* seq_len;
    uint64_t* seq_word_off;
    uint32_t* bases;
    uint32_t group_cap, seq_cap;
    uint64_t word_cap;
    uint32_t* status;        /* [0] = 1 when an output capacity was exceeded, [1] = 1 when the output groups outgrow the working arrays; the totals for the
                                host: [2] output groups, [3] sequences, [4..5] words */
};

/* one work-group: windows per input group and their exclusive prefix sums */
__global__ void __launch_bounds__(1024) cw_cut_index_kernel(CutGroupArgs a) {
    __shared__ uint32_t ps[1024];
    __shared__ uint32_t run;
    const int tid = threadIdx.x;
    if (tid == 0) run = 0;
    __syncthreads();
    for (uint32_t g0 = 0; g0 < a.b.n_windows; g0 += 1024) {
        const uint32_t g = g0 + tid;
        uint32_t T = 0;
        if (g < a.b.n_windows) {
            const uint32_t r = a.b.win_first_seq[g];
            if (r < a.b.win_first_seq[g + 1]) T = cut_windows(a.b.seq_len[r], a.window);
        }
        ps[tid] = T;
        __syncthreads();
        for (int o = 1; o < 1024; o <<= 1) {
            uint32_t v = 0;
            if (tid >= o) v = ps[tid - o];
            __syncthreads();
            ps[tid] += v;
            __syncthreads();
        }
        if (g < a.b.n_windows) a.grp[g] = run + ps[tid] - T;
        __syncthreads();
        if (tid == 0) run += ps[1023];
        __syncthreads();
    }
    if (tid == 0) {
        a.grp[a.b.n_windows] = run;
        if (run > a.out_cap) a.status[1] = 1;
        if (run > a.group_cap) a.status[0] = 1;
    }
}

/* output group w: its input group g (the last with grp[g] <= w: groups without windows share their successor's offset), window t, columns [c0, c1) */
struct CutWindow { uint32_t g, r, q_end, t, T, c0, c1; };
__device__ __forceinline__ CutWindow cut_window_of(const CutGroupArgs& a, uint32_t w) {
    uint32_t lo = 0, hi = a.b.n_windows; /* grp[lo] <= w < grp[hi] */
    while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (a.grp[mid] <= w) lo = mid; else hi = mid; }
    CutWindow cw;
    cw.g = lo; cw.r = a.b.win_first_seq[lo]; cw.q_end = a.b.win_first_seq[lo + 1];
    const uint32_t n = a.b.seq_len[cw.r];
    cw.t = w - a.grp[lo]; cw.T = cut_windows(n, a.window);
    cw.c0 = cw.t * a.window; /* t < T: below n */
    cw.c1 = n - cw.c0 > a.window ? cw.c0 + a.window : n;
    return cw;
}

/* query s's piece of the window when it is a member (length > 0): its row counts, its alignment spans the window, its slot holds the words, the piece lies
   inside the query */
__device__ __forceinline__ uint32_t cut_piece(const CutGroupArgs& a, const CutWindow& cw, uint32_t s, uint32_t* first) {
    const int32_t* row = a.rows + (size_t)s * CW_SW_ROW;
    if (row[CW_SW_STATUS] != CW_SW_ALIGNED || row[CW_SW_SCORE] <= 0 || row[CW_SW_REF_BEGIN] < 0) return 0u;
    if ((uint32_t)row[CW_SW_REF_BEGIN] > cw.c0 || row[CW_SW_REF_END] < 0 || (uint32_t)row[CW_SW_REF_END] < cw.c1 - 1u) return 0u;
    if (!cut_slot_holds(a.cut_off, s, cw.T)) return 0u;
    const uint32_t* slot = a.cuts + a.cut_off[s];
    const uint32_t p0 = slot[cw.t], p1 = slot[cw.t + 1u];
    if (p1 <= p0 || p1 > a.b.seq_len[s]) return 0u;
    *first = p0;
    return p1 - p0;
}

__global__ void __launch_bounds__(256) cw_cut_count_kernel(CutGroupArgs a) {
    const int lane = threadIdx.x & 63;
    const uint32_t n_out = a.grp[a.b.n_windows];
    if (n_out > a.out_cap) return;
    for (uint32_t w = blockIdx.x * 4 + (threadIdx.x >> 6); w < n_out; w += gridDim.x * 4) {
        const CutWindow cw = cut_window_of(a, w);
        uint32_t n_mem = 1u;
        uint64_t words = (cw.c1 - cw.c0 + 15u) / 16u;
        for (uint32_t s0 = cw.r + 1u; s0 < cw.q_end; s0 += 64u) {
            const uint32_t s = s0 + (uint32_t)lane;
            uint32_t first = 0;
            const uint32_t len = s < cw.q_end ? cut_piece(a, cw, s, &first) : 0u;
            n_mem += (uint32_t)__popcll(__ballot(len > 0u));
            words += (uint64_t)(uint32_t)cw_wave_sum((int)((len + 15u) / 16u));
        }
        if (lane == 0) { a.win_seqs[w] = n_mem; a.win_words[w] = words; }
    }
}

__global__ void __launch_bounds__(1024) cw_cut_scan_kernel(CutGroupArgs a) {
    __shared__ uint32_t ps[1024];
    __shared__ unsigned long long pw[1024];
    __shared__ unsigned long long run_w;
    __shared__ uint32_t run_s;
    const int tid = threadIdx.x;
    const uint32_t n_out = a.grp[a.b.n_windows];
    if (n_out > a.out_cap) return;
    if (tid == 0) { run_s = 0; run_w = 0; }
    __syncthreads();
    for (uint32_t w0 = 0; w0 < n_out; w0 += 1024) {
        const uint32_t w = w0 + tid;
        const uint32_t s = w < n_out ? a.win_seqs[w] : 0;
        const unsigned long long x = w < n_out ? a.win_words[w] : 0;
        ps[tid] = s; pw[tid] = x;
        __syncthreads();
        for (int o = 1; o < 1024; o <<= 1) {
            uint32_t vs = 0; unsigned long long vw = 0;
            if (tid >= o) { vs = ps[tid - o]; vw = pw[tid - o]; }
            __syncthreads();
            ps[tid] += vs; pw[tid] += vw;
            __syncthreads();
        }
        if (w < n_out) { a.win_seqs[w] = run_s + ps[tid] - s; a.win_words[w] = run_w + pw[tid] - x; }
        __syncthreads();
        if (tid == 0) { run_s += ps[1023]; run_w += pw[1023]; }
        __syncthreads();
    }
    if (tid == 0) {
        a.win_seqs[n_out] = run_s; a.win_words[n_out] = run_w;
        a.status[2] = n_out; a.status[3] = run_s; a.status[4] = (uint32_t)run_w; a.status[5] = (uint32_t)(run_w >> 32);
        if (run_s > a.seq_cap || run_w > a.word_cap) a.status[0] = 1;
    }
}

/* len bases of src from base pos, packed from word offset wo on: a 16-base word a lane and step, the last word's unused low bits zero */
__device__ __forceinline__ void cut_copy(uint32_t* bases, uint64_t wo, const uint32_t* src, uint32_t pos, uint32_t len, int lane) {
    const uint32_t nw = (len + 15u) / 16u;
    for (uint32_t x = (uint32_t)lane; x < nw; x += 64u) {
        uint32_t out = 0;
        const uint32_t nb = min(16u, len - x * 16u);
        for (uint32_t y = 0; y < nb; ++y) out |= cw_base_at(src, pos + x * 16u + y) << (30 - 2 * y);
        bases[wo + x] = out;
    }
}

__global__ void __launch_bounds__(256) cw_cut_fill_kernel(CutGroupArgs a) {
    const int lane = threadIdx.x & 63;
    const uint32_t n_out = a.grp[a.b.n_windows];
    if (a.status[0] || a.status[1]) return;
    for (uint32_t g = blockIdx.x * 256u + threadIdx.x; g <= a.b.n_windows; g += gridDim.x * 256u) a.grp_first[g] = a.grp[g];
    for (uint32_t w = blockIdx.x * 4 + (threadIdx.x >> 6); w <= n_out; w += gridDim.x * 4) {
        if (w == n_out) { if (lane == 0) a.win_first_seq[w] = a.win_seqs[w]; break; }
        const CutWindow cw = cut_window_of(a, w);
        const uint32_t s_base = a.win_seqs[w];
        uint64_t wo = a.win_words[w];
        if (lane == 0) { a.win_first_seq[w] = s_base; a.seq_len[s_base] = cw.c1 - cw.c0; a.seq_word_off[s_base] = wo; }
        cut_copy(a.bases, wo, a.b.bases + a.b.seq_word_off[cw.r], cw.c0, cw.c1 - cw.c0, lane);
        wo += (cw.c1 - cw.c0 + 15u) / 16u;
        uint32_t n_mem = 1u;
        for (uint32_t s0 = cw.r + 1u; s0 < cw.q_end; s0 += 64u) {
            const uint32_t s = s0 + (uint32_t)lane;
            uint32_t first = 0;
            const uint32_t len = s < cw.q_end ? cut_piece(a, cw, s, &first) : 0u;
            unsigned long long bal = __ballot(len > 0u);
            const uint32_t idx = s_base + n_mem + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
            /* the word offset of a member: the words of the members before it in the round */
            const uint32_t nw = (len + 15u) / 16u;
            const uint32_t before = (uint32_t)cw_wave_scan_add((int)nw) - nw;
            if (len > 0u) { a.seq_len[idx] = len; a.seq_word_off[idx] = wo + before; }
            n_mem += (uint32_t)__popcll(bal);
            while (bal) { /* member by member, the wave on its words */
                const int src = __builtin_ctzll(bal);
                bal &= bal - 1ull;
                const uint32_t m_len = (uint32_t)__shfl((int)len, src), m_first = (uint32_t)__shfl((int)first, src), m_before = (uint32_t)__shfl((int)before, src);
                cut_copy(a.bases, wo + m_before, a.b.bases + a.b.seq_word_off[s0 + (uint32_t)src], m_first, m_len, lane);
            }
            wo += (uint64_t)(uint32_t)cw_lane_value(cw_wave_scan_add((int)nw), 63);
        }
    }
}

#endif
