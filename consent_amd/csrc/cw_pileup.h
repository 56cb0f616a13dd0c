/*
 * cw_pileup.h -- the alignment operator's pileup run (cw_pileup_run / cw_pileup_run_device, include/consent_amd.h): per pair the row of cw_sw_path_run, and
 * instead of the path's ops what the paths say about the reference: eight counts per reference column (A, C, G, T, deletions, insertion events after it,
 * alignments that begin and that end on it).  The kernels are calls of cw_sw_op.h's sw_class_loop / sw_long_loop (LDS slabs, per-wave scratch, pair-claim loop,
 * under the launch bounds of the path kernels) around pile_pair, which follows sw_path_pair line by line up to the closed walk.  The run's own are:
 *
 *   cw_pileup_clear_kernel  one work-group per group: columns 0 .. ref_len - 1 of the group's reference, where its slot holds them, in 16-byte stores (two a
 *                           column).  Not launched under CW_PILE_ACCUMULATE.
 *   pile_count              wave-wide, in place of sw_emit: the walk's steps in alignment order (step k is steps[n - 1 - k]), 64 a round.  (i, j) of a step are
 *                           the prefix sums of what the steps before it consumed, carried from round to round as in sw_emit's EQX branch.  An M step adds one to
 *                           its column's word of the query base, a D step to the column's DEL; an I step counts only when the step before it (steps[n - k], read
 *                           from the buffer: no carry) is not an I, and then adds one to INS of the last column consumed, j - 1.  Integer atomicAdd, result unused.
 *                           Within a round no two lanes hit the same word -- a path consumes a column once, and INS and the base counts are different words --
 *                           so nothing is reduced across the wave first.  Integer adds commute: the counts depend on no batch, wave order or run.
 */
#ifndef CW_PILEUP_H
#define CW_PILEUP_H

#include "cw_sw_path.h"

static_assert(CW_PILE_COL == 8 && CW_PILE_COL * sizeof(uint32_t) == 2 * sizeof(uint4), "a column is two 16-byte stores");
static_assert(CW_PILE_T == 3 && CW_PILE_DEL == 4 && CW_PILE_INS == 5 && CW_PILE_BEGIN == 6 && CW_PILE_END == 7, "a base's word is its packed code");

struct PileArgs {
    SwArgs a;                /* as for cw_sw_path_run: a.dir / a.dir_bytes are CW_SW_PATH_BYTES per wave */
    uint32_t* counts;        /* the caller's, 16-byte aligned */
    const uint64_t* col_off; /* [n_seqs + 1] */
    uint8_t* steps;          /* CW_SW_STEP_BYTES per wave of the largest grid */
};

/* whether sequence r's slot holds the n columns of r as a reference */
__device__ __forceinline__ bool pile_slot_holds(const uint64_t* col_off, uint32_t r, uint32_t n) {
    const uint64_t o0 = col_off[r], o1 = col_off[r + 1];
    return o1 >= o0 && o1 - o0 >= (uint64_t)n;
}

__global__ void __launch_bounds__(256) cw_pileup_clear_kernel(PileArgs pa) {
    const uint32_t g = blockIdx.x;
    if (g >= pa.a.b.n_windows) return;
    const uint32_t r = pa.a.b.win_first_seq[g];
    if (r >= pa.a.b.win_first_seq[g + 1]) return; /* a group of none */
    const uint32_t n = pa.a.b.seq_len[r];
    if (!pile_slot_holds(pa.col_off, r, n)) return;
    uint4* const cols = (uint4*)(pa.counts + pa.col_off[r] * CW_PILE_COL);
    const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
    for (uint32_t x = threadIdx.x; x < 2u * n; x += 256u) cols[x] = zero;
}

/* the counts of n steps of a closed path over ref_span columns; cols: the begin column's words, read: the query from its begin */
__device__ __forceinline__ void pile_count(const uint8_t* steps, uint32_t n, uint32_t ref_span, const uint8_t* read, uint32_t* cols, int lane) {
    uint32_t ci = 0, cj = 0;
    for (uint32_t base = 0; base < n; base += 64u) {
        const uint32_t k = base + (uint32_t)lane;
        const bool on = k < n;
        const int c = on ? (int)steps[n - 1u - k] : 3;
        const int di = on && c != 2 ? 1 : 0, dj = on && c != 1 ? 1 : 0;
        const int si = cw_wave_scan_add(di), sj = cw_wave_scan_add(dj);
        const uint32_t i0 = ci + (uint32_t)(si - di), j0 = cj + (uint32_t)(sj - dj);
        if (on) {
            if (c == 1) { /* the run's first step only; j0 columns are consumed, the last of them j0 - 1 (a path begins with an M: k > 0, j0 > 0) */
                if (k > 0u && steps[n - k] != 1 && j0 > 0u && j0 <= ref_span) atomicAdd(cols + (size_t)(j0 - 1u) * CW_PILE_COL + CW_PILE_INS, 1u);
            } else if (j0 < ref_span) atomicAdd(cols + (size_t)j0 * CW_PILE_COL + (c == 0 ? (uint32_t)(read[i0] & 3u) : (uint32_t)CW_PILE_DEL), 1u);
        }
        ci += (uint32_t)cw_lane_value(si, 63); cj += (uint32_t)cw_lane_value(sj, 63);
    }
    if (lane == 0 && ref_span > 0u) {
        atomicAdd(cols + CW_PILE_BEGIN, 1u);
        atomicAdd(cols + (size_t)(ref_span - 1u) * CW_PILE_COL + CW_PILE_END, 1u);
    }
}

/* one pair on one wave, its buffers in place, as sw_path_pair: align, the banded pass, the walk -- then the counts in place of the ops -- the row */
template <int CLS, bool SPAN>
__device__ __forceinline__ void pile_pair(const PileArgs& pa, uint32_t s, uint8_t* refc, uint8_t* qfw, uint8_t* qrv, uint32_t qrv_bytes, bool qrv_lds, uint8_t* rows, uint8_t* dirbuf, uint8_t* steps,
                                          uint8_t* state, int lane) {
    const SwArgs& a = pa.a;
    const uint32_t r = st_uni(a.seq_ref[s]);
    const uint32_t m = st_uni(a.b.seq_len[s]), n = st_uni(a.b.seq_len[r]);
    const uint32_t sn = sw_unpack_ref<SPAN>(a, refc, s, r, n, lane);
    sw_unpack(qfw, a.b.bases + a.b.seq_word_off[s], m, lane);
    st_mem_sync();
    const StAlign al = sw_align<CLS>(qfw, (int)m, qrv, refc, (int)sn, lane, state); /* in the span's coordinates, as everything up to the walk */
    uint32_t ins = 0, del = 0;
    int status = CW_SW_ALIGNED;
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
                if (!pile_slot_holds(pa.col_off, r, n) || al.ref_begin < 0 || (uint32_t)al.ref_begin + (uint32_t)refLen > sl.len) status = CW_SW_PILE_SLOT; /* (the ends lie inside the span, the span inside the reference) */
                else pile_count(steps, w.n_steps, (uint32_t)refLen, read0, pa.counts + (pa.col_off[r] + (uint64_t)sl.lo + (uint64_t)al.ref_begin) * CW_PILE_COL, lane); /* columns are absolute */
            }
        }
    }
    if (lane == 0) {
        const int lo = al.score > 0 ? (int)sw_pair_lo<SPAN>(a, s) : 0; /* the row is absolute */
        sw_write_row(a.rows + (size_t)s * CW_SW_ROW, al.score, al.ref_begin + lo, al.ref_end + lo, al.query_begin, al.query_end, ins, del, status);
    }
    st_mem_sync(); /* the next pair's unpacking overwrites what this one read */
}

template <int CLS, bool SPAN>
__global__ void __launch_bounds__(64 * CW_SW_WAVES, CLS == 0 ? 4 : 1) cw_pileup_kernel(PileArgs pa) {
    sw_class_loop<CLS, true, SPAN>(pa.a, pa.steps, [&](uint32_t s, const SwWaveBufs& w, int lane) __attribute__((always_inline)) {
        pile_pair<CLS, SPAN>(pa, s, w.refc, w.qfw, w.qrv, w.qrv_bytes, w.qrv_lds, w.rows, w.dirbuf, w.steps, w.state, lane);
    });
}

template <bool SPAN>
__global__ void __launch_bounds__(64, 2) cw_pileup_long_kernel(PileArgs pa) {
    sw_long_loop<true>(pa.a, pa.steps, [&](uint32_t s, const SwWaveBufs& w, int lane) __attribute__((always_inline)) {
        pile_pair<2, SPAN>(pa, s, w.refc, w.qfw, w.qrv, w.qrv_bytes, w.qrv_lds, w.rows, w.dirbuf, w.steps, w.state, lane);
    });
}

#endif
