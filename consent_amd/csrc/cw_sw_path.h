/*
 * cw_sw_path.h -- the alignment operator's path run (cw_sw_path_run / cw_sw_path_run_device, include/consent_amd.h): per pair the row of cw_sw_run and the
 * alignment itself as run-length encoded ops.  One wave per pair, the order kernel, the unpacking, the sweeps and the three launch classes of cw_sw_op.h; new are
 * the traceback behind them and its kernels, which are calls of cw_sw_op.h's sw_class_loop / sw_long_loop.  cw_stitch.h is not edited: cw_sw_run and the
 * re-assembly keep st_banded_indels.  The pileup and cut runs (cw_pileup.h, cw_sw_cut.h) use sw_banded_path and sw_walk from here; their pair bodies
 * (pile_pair, cut_pair) are copies of sw_path_pair up to the closed walk: one shared body with a sink per run compiled to other registers and spills.
 *
 *   sw_banded_path   ssw's banded pass between the found ends (oracle/cw_oracle.cpp ssw_banded_indels), its rows on the lanes for EVERY band width: a row of the
 *                    band goes in chunks of 64 cells, lowest first.  The arrays h_b / e_b / h_c and their index rules -- the zeroed `edge` slots, the shift
 *                    between a row's own index u and the row before's e, whatever an earlier row left beyond the cells of the last one -- are those of the
 *                    serial loop.  The in-row gap is the exclusive prefix maximum of st_banded_indels' narrow path (exact: open >= ext, no cell negative), its
 *                    running maximum and the last cell's h / f carried from chunk to chunk.  Order: a chunk reads e_b / h_b at e = j - xp + 1 and writes
 *                    e_b[u], u = j - xo + 1 <= e (xp <= xo), always below what the chunks after it read (their e is larger than this chunk's largest u); h_b is
 *                    read at e and e - 1, which reaches this row's u of the chunk before -- so h_b is replaced only after the whole row, from h_c.
 *                    Directions: ONE byte a cell (bit 0: E opened, bit 1: F opened, bits 2-3: H took 1 = diagonal, 2 = E, 3 = F; 0 = no cell: stop), every
 *                    row written to its full stride, so nothing is cleared beforehand.
 *   sw_walk          one lane (a chain of dependent one-byte reads): from the end cell in state H, one step code (0 M, 1 I, 2 D) a step into the wave's step
 *                    buffer; closed as ssw closes it -- the walk stops at query row 0, and that row's cell is one more M.
 *   sw_emit          wave-wide: the steps in alignment order, run ends by ballot, positions by popcount over rounds of 64 steps; under CW_SW_PATH_EQX an M step
 *                    is '=' or 'X' by its bases, its (i, j) the prefix sums of what the steps before it consumed.  A counting pass first: the size check
 *                    against the caller's slot precedes the first store.
 */
#ifndef CW_SW_PATH_H
#define CW_SW_PATH_H

#include "cw_sw_op.h"

#define CW_SW_PATH_MAX_WAVES 512u /* x CW_SW_PATH_BYTES = the 1 GiB of direction scratch an indel run plans at most */

static_assert(CW_SW_QMAX + CW_SW_RMAX <= CW_SW_STEP_BYTES, "every step consumes a base of the query or of the reference");
static_assert(CW_SW_PATH_BYTES == 2u * CW_ST_DIR_BYTES, "a byte a cell, in twice the indel run's scratch");
static_assert((uint64_t)CW_SW_PATH_MAX_WAVES * CW_SW_PATH_BYTES == (uint64_t)CW_ST_MAX_WGS * CW_ST_WAVES * CW_ST_DIR_BYTES, "the direction scratch of a run: what plan_sw holds under CW_SW_WANT_INDELS");

struct SwPathArgs {
    SwArgs a;                /* as for cw_sw_run; a.dir / a.dir_bytes: CW_SW_PATH_BYTES per wave */
    uint32_t* ops;           /* the caller's */
    const uint64_t* ops_off; /* [n_seqs + 1] */
    uint32_t* n_ops;         /* [n_seqs], zero before the launches */
    uint8_t* steps;          /* CW_SW_STEP_BYTES per wave of the largest grid */
};

struct SwBand { int band, stride; const uint8_t* dir; bool fits; };

__device__ __forceinline__ SwBand sw_banded_path(const uint8_t* ref, int refLen, const uint8_t* read, int readLen, int score, uint8_t* rows, uint8_t* dir_all, uint32_t dir_bytes,
                                                 uint8_t* dir_lds, uint32_t dir_lds_bytes, int lane) {
    const int GO = CW_SSW_GAP_OPEN, GE = CW_SSW_GAP_EXT;
    int band = abs(refLen - readLen) + 1;
    for (;;) {
        const int width = band * 2 + 3, width_d = band * 2 + 1;
        /* a band wider than the matrix only ever touches refLen + 1 cells per row (st_banded_indels) */
        const int w_rows = width < refLen + 3 ? width : refLen + 3;
        const int stride = width_d < refLen + 1 ? width_d : refLen + 1;
        const size_t rows_need = (size_t)w_rows * 12, dir_need = (size_t)stride * readLen;
        const bool rows_in_lds = rows_need <= CW_ST_ROWS_BYTES;
        const size_t rows_glb = rows_in_lds ? 0 : ((rows_need + 15) & ~(size_t)15);
        if (dir_need + rows_glb > dir_bytes) return SwBand{band, stride, nullptr, false};
        int* const h_b = rows_in_lds ? (int*)rows : (int*)dir_all; int* const e_b = h_b + w_rows; int* const h_c = e_b + w_rows;
        uint8_t* const dir = rows_in_lds && dir_need <= dir_lds_bytes ? dir_lds : dir_all + rows_glb;
        for (int x = lane; x < 3 * w_rows; x += 64) h_b[x] = 0; /* h_b, e_b, h_c are one block */
        int mx = 0;
        const int n_chunks = (stride + 63) >> 6;
        for (int i = 0; i < readLen; ++i) {
            int beg = i - band, end = i + band;
            beg = beg > 0 ? beg : 0; end = end < refLen - 1 ? end : refLen - 1;
            const int edge = end + 1 < width - 1 ? end + 1 : width - 1;
            if (lane == 0) { h_b[0] = 0; e_b[0] = 0; h_b[edge] = 0; e_b[edge] = 0; h_c[0] = 0; }
            st_mem_sync();
            const int xo = beg, xp = i - 1 - band > 0 ? i - 1 - band : 0; /* (max(i - band, 0) is beg) */
            const int bq = st_uni((int)read[i]);
            uint8_t* const line = dir + (size_t)stride * i;
            unsigned carry_key = 0u; /* far below anything */
            int carry_hc = 0, carry_f = 0; /* h_c[0] = 0 and f = 0 before the first cell */
            bool on = false; int u = 0, hc = 0; /* (after the loop: the last chunk's, the row's only one when n_chunks == 1) */
            for (int c = 0; c < n_chunks; ++c) {
                const int tg = 64 * c + lane, j = beg + tg;
                on = j <= end;
                u = j - xo + 1;
                const int e_i = j - xp + 1;
                int hbe = 0, ebe = 0, hbd = 0, a = 4;
                if (on) { hbe = h_b[e_i]; ebe = e_b[e_i]; hbd = h_b[e_i - 1]; a = ref[j]; }
                const int t1e = i == 0 ? -GO : hbe - GO, t2e = i == 0 ? -GE : ebe - GE;
                const int e_new = t1e > t2e ? t1e : t2e;
                const int e_open = t1e > t2e ? 1 : 0;
                const int e1 = e_new > 0 ? e_new : 0;
                const int diag = hbd + ((a == 4 || bq == 4) ? 0 : (a == bq ? CW_SSW_MATCH : -CW_SSW_MISMATCH));
                const int hq = e1 > diag ? e1 : diag;
                const unsigned key = on ? (unsigned)(hq - GO + (tg + 1) * GE + 0x40000000) : 0u;
                const unsigned inc = cw_wave_scan_max_u32(key);
                const unsigned exu = max((unsigned)CW_DPP((int)carry_key, (int)inc, 0x138, 0xF), carry_key);
                const int ex = (int)exu - 0x40000000;
                const int f = (ex > -GE ? ex : -GE) - tg * GE;
                const int f1 = f > 0 ? f : 0;
                const int t1h = e1 > f1 ? e1 : f1;
                hc = t1h > diag ? t1h : diag;
                const int hc_prev = CW_DPP(carry_hc, hc, 0x138, 0xF), f_prev = CW_DPP(carry_f, f, 0x138, 0xF);
                const int f_open = hc_prev - GO > f_prev - GE ? 1 : 0;
                const int dir_h = t1h <= diag ? 1 : (e1 > f1 ? 2 : 3);
                if (on) { e_b[u] = e_new; if (n_chunks > 1) h_c[u] = hc; mx = hc > mx ? hc : mx; }
                if (tg < stride) line[tg] = on ? (uint8_t)(e_open | (f_open << 1) | (dir_h << 2)) : (uint8_t)0; /* cells outside the band read as "stop" */
                carry_key = max(carry_key, (unsigned)cw_lane_value((int)inc, 63));
                carry_hc = cw_lane_value(hc, 63); carry_f = cw_lane_value(f, 63); /* (read only when a chunk follows a full one) */
            }
            st_mem_sync();
            /* for (j = 1; j <= u; ++j) h_b[j] = h_c[j]: a row of one chunk has its cells in registers still (h_c itself is read by nothing else) */
            if (n_chunks == 1) { if (on) h_b[u] = hc; }
            else { const int u_last = end - xo + 1; for (int x = 1 + lane; x <= u_last; x += 64) h_b[x] = h_c[x]; }
        }
        mx = st_uni(cw_wave_max(mx));
        st_mem_sync();
        if (mx >= score || band > refLen + readLen) return SwBand{band, stride, dir, true};
        band *= 2;
    }
}

struct SwWalk { uint32_t n_steps, ins, del; bool closed; };

/* lane 0 walks; every lane returns the same numbers.  steps[] in walk order (end to begin). */
__device__ __forceinline__ SwWalk sw_walk(const SwBand& bd, int refLen, int readLen, uint8_t* steps, int lane) {
    unsigned n = 0, ni = 0, nd = 0, closed = 0;
    if (lane == 0) {
        const int band = bd.band, width_d = 2 * bd.band + 1;
        int i = readLen - 1, j = refLen - 1, state = 2;
        bool left = false;
        while (i > 0 && j >= 0) {
            int x = i - band; x = x > 0 ? x : 0; x = j - x;
            if (x < 0 || x >= width_d) { left = true; break; } /* (x <= j < the stride) */
            const unsigned b = bd.dir[(size_t)bd.stride * i + x];
            if (b == 0u) { left = true; break; } /* outside the band */
            const unsigned dh = b >> 2;
            const unsigned via = state == 2 ? dh : state == 0 ? 2u : 3u; /* 1: diagonal, 2: the E code, 3: the F code */
            if (via == 1u) { --i; --j; state = 2; steps[n++] = 0; }
            else if (via == 2u) { --i; state = (b & 1u) ? 2 : 0; ++ni; steps[n++] = 1; }
            else { --j; state = (b & 2u) ? 2 : 1; ++nd; steps[n++] = 2; }
        }
        if (!left && i == 0 && j == 0) { closed = 1; steps[n++] = 0; }
    }
    SwWalk w;
    w.n_steps = (uint32_t)cw_lane_value((int)n, 0); w.ins = (uint32_t)cw_lane_value((int)ni, 0); w.del = (uint32_t)cw_lane_value((int)nd, 0);
    w.closed = cw_lane_value((int)closed, 0) != 0;
    st_mem_sync();
    return w;
}

/* the ops of n steps; WRITE = false only counts them.  ref / read begin at the alignment's begin cell. */
template <bool WRITE>
__device__ __forceinline__ uint32_t sw_emit(const uint8_t* steps, uint32_t n, bool eqx, const uint8_t* ref, const uint8_t* read, uint32_t* out, int lane) {
    uint32_t n_ops = 0, ci = 0, cj = 0;
    int last_end = -1; /* the step the run before the present one ended at */
    for (uint32_t base = 0; base < n; base += 64u) {
        const uint32_t k = base + (uint32_t)lane;
        const bool on = k < n, more = k + 1u < n;
        int c = on ? (int)steps[n - 1u - k] : 3, c1 = more ? (int)steps[n - 2u - k] : 3;
        if (eqx) {
            const int di = on && c != 2 ? 1 : 0, dj = on && c != 1 ? 1 : 0;
            const int si = cw_wave_scan_add(di), sj = cw_wave_scan_add(dj);
            const uint32_t i0 = ci + (uint32_t)(si - di), j0 = cj + (uint32_t)(sj - dj);
            if (on && c == 0) c = read[i0] == ref[j0] ? 7 : 8;
            if (more && c1 == 0) c1 = read[i0 + (uint32_t)di] == ref[j0 + (uint32_t)dj] ? 7 : 8;
            ci += (uint32_t)cw_lane_value(si, 63); cj += (uint32_t)cw_lane_value(sj, 63);
        }
        const bool is_end = on && c1 != c; /* (the last step: c1 = 3, no code) */
        const unsigned long long ends = __ballot(is_end);
        if (WRITE) {
            const unsigned long long below = ends & ((1ull << lane) - 1ull);
            if (is_end) {
                const int prev = below ? (int)base + 63 - (int)__builtin_clzll(below) : last_end;
                out[n_ops + (uint32_t)__builtin_popcountll(below)] = ((uint32_t)((int)k - prev) << 4) | (uint32_t)c;
            }
            if (ends) last_end = (int)base + 63 - (int)__builtin_clzll(ends);
        }
        n_ops += (uint32_t)__builtin_popcountll(ends);
    }
    return n_ops;
}

/* one pair on one wave, its buffers in place: align, the banded pass, the walk, the ops, the row */
template <int CLS, bool SPAN>
__device__ __forceinline__ void sw_path_pair(const SwPathArgs& pa, uint32_t s, uint8_t* refc, uint8_t* qfw, uint8_t* qrv, uint32_t qrv_bytes, bool qrv_lds, uint8_t* rows, uint8_t* dirbuf, uint8_t* steps,
                                             uint8_t* state, int lane) {
    const SwArgs& a = pa.a;
    const uint32_t r = st_uni(a.seq_ref[s]);
    const uint32_t m = st_uni(a.b.seq_len[s]), n = st_uni(a.b.seq_len[r]);
    const uint32_t sn = sw_unpack_ref<SPAN>(a, refc, s, r, n, lane);
    sw_unpack(qfw, a.b.bases + a.b.seq_word_off[s], m, lane);
    st_mem_sync();
    const StAlign al = sw_align<CLS>(qfw, (int)m, qrv, refc, (int)sn, lane, state); /* in the span's coordinates, as everything up to the walk */
    uint32_t ins = 0, del = 0, n_ops = 0;
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
                const bool eqx = (a.flags & CW_SW_PATH_EQX) != 0u;
                const uint64_t o0 = pa.ops_off[s], o1 = pa.ops_off[s + 1];
                n_ops = sw_emit<false>(steps, w.n_steps, eqx, ref0, read0, nullptr, lane);
                if (o1 < o0 || (uint64_t)n_ops > o1 - o0) status = CW_SW_PATH_SLOT;
                else sw_emit<true>(steps, w.n_steps, eqx, ref0, read0, pa.ops + o0, lane);
            }
        }
    }
    if (lane == 0) {
        const int lo = al.score > 0 ? (int)sw_pair_lo<SPAN>(a, s) : 0; /* the row is absolute */
        sw_write_row(a.rows + (size_t)s * CW_SW_ROW, al.score, al.ref_begin + lo, al.ref_end + lo, al.query_begin, al.query_end, ins, del, status);
        pa.n_ops[s] = n_ops;
    }
    st_mem_sync(); /* the next pair's unpacking overwrites what this one read */
}

/* the launch bounds and LDS slabs of cw_sw_kernel<CLS> */
template <int CLS, bool SPAN>
__global__ void __launch_bounds__(64 * CW_SW_WAVES, CLS == 0 ? 4 : 1) cw_sw_path_kernel(SwPathArgs pa) {
    sw_class_loop<CLS, true, SPAN>(pa.a, pa.steps, [&](uint32_t s, const SwWaveBufs& w, int lane) __attribute__((always_inline)) {
        sw_path_pair<CLS, SPAN>(pa, s, w.refc, w.qfw, w.qrv, w.qrv_bytes, w.qrv_lds, w.rows, w.dirbuf, w.steps, w.state, lane);
    });
}

template <bool SPAN>
__global__ void __launch_bounds__(64, 2) cw_sw_path_long_kernel(SwPathArgs pa) {
    sw_long_loop<true>(pa.a, pa.steps, [&](uint32_t s, const SwWaveBufs& w, int lane) __attribute__((always_inline)) {
        sw_path_pair<2, SPAN>(pa, s, w.refc, w.qfw, w.qrv, w.qrv_bytes, w.qrv_lds, w.rows, w.dirbuf, w.steps, w.state, lane);
    });
}

#endif
