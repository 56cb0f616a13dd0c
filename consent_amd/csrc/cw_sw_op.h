/*
 * cw_sw_op.h -- the re-assembly's local aligner as a batched operator (cw_sw_run / cw_sw_run_device, include/consent_amd.h): one wave per
 * (query, reference) pair around the device functions of cw_stitch.h (st_align over the striped register sweeps and st_sweep_mem, st_banded_indels),
 * which are unchanged -- and so is cw_stitch_kernel.
 *
 *   cw_sw_order_kernel  three small launches (phase 0, 1, 2) over the sequences of the batch: a sequence's reference is its group's first sequence; rows that
 *                       need no alignment (the reference's own, a pair beyond a capacity, an empty query or reference) are written at once; the others are
 *                       pairs, counted per (launch class, cost class) and handed out costliest first -- a launch lasts as long as its last-started long pair
 *                       (cw_stitch_order_kernel's reason).  Launch classes: 0 = query of at most CW_SW_Q0 bases (sweeps of 1..5 registers a slot: 128 registers,
 *                       four waves a SIMD), 1 = up to CW_ST_QMAX (the full ladder: one wave a SIMD), 2 = up to CW_STH_QMAX (st_sweep_mem, state in global memory).
 *   cw_sw_kernel<CLS>   classes 0 and 1: query codes and the reversed prefix in the wave's LDS slab, the reference there too up to CW_ST_RMAX bases and in the
 *                       wave's global scratch beyond; st_align, then under CW_SW_WANT_INDELS st_banded_indels (rows in LDS, directions in the wave's
 *                       CW_ST_DIR_BYTES of global scratch), then the row.
 *   cw_sw_long_kernel   class 2: one wave a work-group, every buffer and the sweep's state in the wave's global scratch (CW_SW_LONG_WAVE_BYTES); always
 *                       enqueued, ends at once when the order kernel counted no such pair.
 *
 * The three alignment launches run one after the other on one stream, so they share the per-wave direction scratch and reference scratch.  cw_plan.h plan_sw
 * sizes everything; cw_engine.cpp run_sw_locked launches by it.
 *
 * The path, pileup and cut runs (cw_sw_path.h, cw_pileup.h, cw_sw_cut.h) launch kernels of their own names in the same three classes.  What the four runs'
 * kernels share lives here, once: sw_class_loop<CLS> and sw_long_loop carve a wave's buffers (SwWaveBufs) and claim the pairs; every kernel is a call of one
 * of the two with what it does per pair.
 *
 * Every alignment kernel has two instances, SPAN = false and SPAN = true (cw_sw_span_run and its kin: a query confined to a span of its reference's columns;
 * SwSpan below).  The first is the kernel as it always was.
 */
#ifndef CW_SW_OP_H
#define CW_SW_OP_H

#include "cw_device.h"
#include "cw_stitch.h"

#define CW_SW_WAVES 4            /* waves per work-group of cw_sw_kernel */
#define CW_SW_Q0 640             /* longest query of launch class 0: st_sweep_any's five-register sweep */
#define CW_SW_GREF_BYTES 16384u  /* a reference beyond CW_ST_RMAX bases, unpacked: per wave, global (CW_SW_RMAX codes and the slack of whole words) */
#define CW_SW_COST_CLASSES 128   /* four per power of two of query length x reference length */
#define CW_SW_CTR_WORDS (8 + 3 * CW_SW_COST_CLASSES) /* cursors [0..2], pairs per launch class [3..5], then the classes' counts / offsets */
#define CW_SW_LONG_MAX_WGS 256
#define CW_SW_STEP_BYTES 49152u  /* a traced run's walk (cw_sw_path.h), per wave: at most query span + reference span steps */
/* the long launch, per wave: reference codes | query codes | reversed prefix | the sweep's state */
#define CW_SW_LONG_WAVE_BYTES ((size_t)CW_SW_GREF_BYTES + 2 * (size_t)CW_STH_QMAX + CW_STH_STATE_BYTES)
/* per wave of cw_sw_kernel: reference codes | query codes | reversed prefix (and the traceback's directions when they are few) | traceback rows */
#define CW_SW_SLAB_OF(QMAX) (CW_ST_RMAX + 2 * (QMAX) + CW_ST_ROWS_BYTES)

static_assert(CW_SW_RMAX <= 16383, "a score is at most 2 x min(query, reference) and lives in a signed 16-bit half, as a column does");
static_assert(((CW_SW_RMAX + 15) & ~15) <= CW_SW_GREF_BYTES && CW_SW_RMAX >= CW_ST_RMAX, "the unpacked reference and the words' slack fit the wave's scratch");
static_assert(CW_SW_DIR_BYTES == CW_ST_DIR_BYTES, "the per-wave traceback scratch is the stitch's");
static_assert(CW_SW_QMAX == CW_STH_QMAX, "the header's query capacity is what st_sweep_mem holds");
static_assert(CW_SW_Q0 % 16 == 0 && CW_ST_QMAX % 16 == 0 && CW_ST_RMAX % 16 == 0 && CW_STH_QMAX % 16 == 0, "sequences are unpacked a word of 16 bases at a time");
static_assert((uint64_t)CW_SW_QMAX * CW_SW_RMAX < (1ull << 30), "a pair's cost in 32 bits");

struct SwArgs {
    DevBatch b;          /* the groups */
    uint32_t n_seqs;
    int32_t* rows;       /* the caller's [n_seqs * CW_SW_ROW] */
    uint32_t flags;
    uint32_t* ctr;       /* CW_SW_CTR_WORDS, zero before phase 0 */
    uint32_t* seq_ref;   /* [3 n_seqs] a pair's reference sequence (phase 0); a span run: behind those its span's first column, behind those its span's columns */
    uint32_t* order;     /* [n_seqs] the pairs: class 0's, then class 1's, then class 2's, each costliest first (phase 2) */
    int8_t* dir;         /* dir_bytes per wave of the largest grid; NULL without CW_SW_WANT_INDELS */
    uint32_t dir_bytes;
    uint8_t* gref;       /* CW_SW_GREF_BYTES per wave of cw_sw_kernel's largest grid */
    uint8_t* lstate;     /* CW_SW_LONG_WAVE_BYTES per work-group of cw_sw_long_kernel */
    const uint32_t* ref_lo; /* [n_seqs] the span runs (cw_sw_span_run and its kin): the reference columns [ref_lo[s], ref_hi[s]) query s may use, clamped */
    const uint32_t* ref_hi; /*          to the reference; both NULL for the runs without spans: every column.  Only the order kernel reads them */
};

/* A pair's span: its first reference column and its columns.  (0, n) without spans; len = 0 when the clamped span is empty.  Everything between the unpacking
   and the row is in span-relative coordinates: the unpacked reference begins at lo.  In a span run the order kernel works a span out once (sw_span_of) and
   leaves it behind the pair's reference in seq_ref[]; the alignment kernels read it there (sw_pair_lo, sw_pair_len) where they need it and keep nothing of it
   in a register across the sweeps: with the caller's two pointers and a recomputation in the pair, the 128-register kernels spilled scalar registers
   (DESIGN.md 4.8 has the table).  A run without spans touches none of this: its kernels are the SPAN = false instances, compiled to the code they always
   were; a span run launches the SPAN = true instances of the same functions.  (One set of kernels for both, with a wave-uniform test a pair, leaves the runs
   without spans with more scalar registers and spills and a path run 3 to 6 % slower at short queries: DESIGN.md 4.8 has the measurements.) */
struct SwSpan { uint32_t lo, len; };
__device__ __forceinline__ SwSpan sw_span_of(const SwArgs& a, uint32_t s, uint32_t n) {
    if (!a.ref_lo) return SwSpan{0u, n};
    const uint32_t lo = min(a.ref_lo[s], n), hi = min(a.ref_hi[s], n);
    return SwSpan{lo, hi > lo ? hi - lo : 0u};
}
/* a pair's span as the order kernel left it; n: its reference's length */
template <bool SPAN>
__device__ __forceinline__ uint32_t sw_pair_lo(const SwArgs& a, uint32_t s) { if constexpr (SPAN) return a.seq_ref[(size_t)a.n_seqs + s]; else return 0u; }
template <bool SPAN>
__device__ __forceinline__ uint32_t sw_pair_len(const SwArgs& a, uint32_t s, uint32_t n) { if constexpr (SPAN) return a.seq_ref[2u * (size_t)a.n_seqs + s]; else return n; }

__device__ __forceinline__ uint32_t sw_launch_class(uint32_t m) { return m <= (uint32_t)CW_SW_Q0 ? 0u : m <= (uint32_t)CW_ST_QMAX ? 1u : 2u; }
/* cost class of a pair of m x n cells, both > 0: 4 x floor(log2) + the next two bits -- monotone in the cost */
__device__ __forceinline__ uint32_t sw_cost_class(uint32_t m, uint32_t n) {
    const uint32_t c = m * n;
    const uint32_t lg = 31u - (uint32_t)__builtin_clz(c);
    const uint32_t frac = lg >= 2u ? (c >> (lg - 2u)) & 3u : 0u;
    return lg * 4u + frac; /* < 4 * 30 + 4 */
}

__device__ __forceinline__ void sw_write_row(int32_t* row, int score, int rb, int re, int qb, int qe, unsigned ins, unsigned del, int status) {
    row[CW_SW_SCORE] = score; row[CW_SW_REF_BEGIN] = rb; row[CW_SW_REF_END] = re; row[CW_SW_QUERY_BEGIN] = qb; row[CW_SW_QUERY_END] = qe;
    row[CW_SW_INS] = (int32_t)ins; row[CW_SW_DEL] = (int32_t)del; row[CW_SW_STATUS] = status;
}

/* phase 0: one thread per sequence -- its group by bisection, its row if that needs no alignment, its class count otherwise
   phase 1: one work-group -- the classes' offsets in order[], launch class by launch class, costliest first; pairs per launch class
   phase 2: one thread per sequence -- a pair takes the next place of its class */
__global__ void __launch_bounds__(256) cw_sw_order_kernel(SwArgs a, int phase) {
    uint32_t* const cls_ctr = a.ctr + 8;
    if (phase == 1) {
        if (threadIdx.x == 0 && blockIdx.x == 0) {
            uint32_t run = 0;
            for (int lc = 0; lc < 3; ++lc) {
                const uint32_t before = run;
                for (int c = CW_SW_COST_CLASSES - 1; c >= 0; --c) { const uint32_t k = cls_ctr[lc * CW_SW_COST_CLASSES + c]; cls_ctr[lc * CW_SW_COST_CLASSES + c] = run; run += k; }
                a.ctr[3 + lc] = run - before;
            }
        }
        return;
    }
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    if (s >= a.n_seqs) return;
    if (phase == 0) {
        /* the group of s: the last g with win_first_seq[g] <= s (empty groups share their successor's first sequence) */
        uint32_t lo = 0, hi = a.b.n_windows; /* win_first_seq[lo] <= s < win_first_seq[hi] = n_seqs */
        while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (a.b.win_first_seq[mid] <= s) lo = mid; else hi = mid; }
        const uint32_t r = a.b.win_first_seq[lo];
        const uint32_t m = a.b.seq_len[s], n = a.b.seq_len[r];
        int32_t* row = a.rows + (size_t)s * CW_SW_ROW;
        a.seq_ref[s] = 0xFFFFFFFFu;
        if (s == r) { sw_write_row(row, 0, 0, -1, 0, -1, 0, 0, CW_SW_IS_REF); return; }
        /* the sweep's capacity is the span's: a span run takes a reference of any length that a row's 32 bits hold */
        const SwSpan sp = sw_span_of(a, s, n);
        const uint32_t sn = sp.len;
        if (m > (uint32_t)CW_SW_QMAX || sn > (uint32_t)CW_SW_RMAX || n > 0x7FFFFFFFu) { sw_write_row(row, 0, 0, -1, 0, -1, 0, 0, CW_SW_STOP); return; }
        if (m == 0u || sn == 0u) { sw_write_row(row, 0, 0, -1, 0, -1, 0, 0, CW_SW_ALIGNED); return; }
        a.seq_ref[s] = r;
        if (a.ref_lo) { a.seq_ref[(size_t)a.n_seqs + s] = sp.lo; a.seq_ref[2u * (size_t)a.n_seqs + s] = sn; }
        atomicAdd(&cls_ctr[sw_launch_class(m) * CW_SW_COST_CLASSES + sw_cost_class(m, sn)], 1u);
        return;
    }
    const uint32_t r = a.seq_ref[s];
    if (r == 0xFFFFFFFFu) return;
    const uint32_t m = a.b.seq_len[s], sn = a.ref_lo ? a.seq_ref[2u * (size_t)a.n_seqs + s] : a.b.seq_len[r];
    a.order[atomicAdd(&cls_ctr[sw_launch_class(m) * CW_SW_COST_CLASSES + sw_cost_class(m, sn)], 1u)] = s;
}

/* 2-bit words to one code a byte, a word of 16 bases per lane and step; writes whole words: dst holds len rounded up to 16 */
__device__ __forceinline__ void sw_unpack(uint8_t* dst, const uint32_t* words, uint32_t len, int lane) {
    const uint32_t nw = (len + 15u) >> 4;
    for (uint32_t w = (uint32_t)lane; w < nw; w += 64u) {
        const uint32_t x = words[w];
        uint32_t* d = (uint32_t*)(dst + 16u * w);
#pragma unroll
        for (int k = 0; k < 4; ++k) { /* bases 4k .. 4k+3 of the word: its byte 3-k, most significant pair first */
            const uint32_t by = (x >> (24 - 8 * k)) & 0xFFu;
            d[k] = ((by >> 6) & 3u) | (((by >> 4) & 3u) << 8) | (((by >> 2) & 3u) << 16) | ((by & 3u) << 24);
        }
    }
}

/* The same from a base that need not begin a word: codes first_base .. first_base + len - 1 of a sequence to dst[0 ..), 16 a lane and step, every output
   word a funnel shift over two neighbouring packed words.  The second of them is loaded only where one of the len codes lies in it -- so it is a word of the
   sequence: nothing beyond the sequence's last word, which may be the batch's last, is ever read.  Writes whole words as sw_unpack does; what lies in dst
   beyond len are the sequence's next bases or zeros, not padding a reader may rely on.  first_base % 16 == 0: the words sw_unpack reads, code for code. */
__device__ __forceinline__ void sw_unpack_from(uint8_t* dst, const uint32_t* words, uint32_t first_base, uint32_t len, int lane) {
    const uint32_t nw = (len + 15u) >> 4, sh = (first_base & 15u) * 2u;
    const uint32_t* const src = words + (first_base >> 4);
    const uint32_t reach = len + (first_base & 15u); /* the codes wanted end at bit pair `reach` of src[] */
    for (uint32_t w = (uint32_t)lane; w < nw; w += 64u) {
        uint32_t x = src[w]; /* (16 w < len: its first code is wanted) */
        if (sh) x = (x << sh) | ((16u * (w + 1u) < reach ? src[w + 1u] : 0u) >> (32u - sh));
        uint32_t* d = (uint32_t*)(dst + 16u * w);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t by = (x >> (24 - 8 * k)) & 0xFFu;
            d[k] = ((by >> 6) & 3u) | (((by >> 4) & 3u) << 8) | (((by >> 2) & 3u) << 16) | ((by & 3u) << 24);
        }
    }
}

/* a pair's reference columns to refc, and their number: the whole reference by sw_unpack as ever, or in a span run its span */
template <bool SPAN>
__device__ __forceinline__ uint32_t sw_unpack_ref(const SwArgs& a, uint8_t* refc, uint32_t s, uint32_t r, uint32_t n, int lane) {
    const uint32_t* const words = a.b.bases + a.b.seq_word_off[r];
    if constexpr (!SPAN) { sw_unpack(refc, words, n, lane); return n; }
    const uint32_t sn = st_uni(sw_pair_len<true>(a, s, n));
    sw_unpack_from(refc, words, st_uni(sw_pair_lo<true>(a, s)), sn, lane);
    return sn;
}

/* the sweeps of a launch class: class 0 is st_sweep_any's ladder up to its five-register instance (what a 128-register kernel holds), class 1 the whole
   ladder, class 2 the last launch's (st_sweep_mem beyond 640 positions) */
template <int CLS, bool TERM>
__device__ __forceinline__ StSweep sw_sweep(const uint8_t* q, int m, const uint8_t* r, int r_first, int r_last_excl, int step, int terminate, int lane, uint8_t* state) {
    if constexpr (CLS == 2) return st_sweep_any<true, TERM>(q, m, r, r_first, r_last_excl, step, terminate, lane, state);
    else if constexpr (CLS == 1) return st_sweep_any<false, TERM>(q, m, r, r_first, r_last_excl, step, terminate, lane, state);
    else {
        m = st_uni(m);
        if (m <= 128) return st_sweep_st2<1, TERM>(q, m, r, r_first, r_last_excl, step, terminate, lane);
        if (m <= 256) return st_sweep_st2<2, TERM>(q, m, r, r_first, r_last_excl, step, terminate, lane);
        if (m <= 384) return st_sweep_st2<3, TERM>(q, m, r, r_first, r_last_excl, step, terminate, lane);
        if (m <= 512) return st_sweep_st2<4, TERM>(q, m, r, r_first, r_last_excl, step, terminate, lane);
        return st_sweep_st2<5, TERM>(q, m, r, r_first, r_last_excl, step, terminate, lane);
    }
}

/* st_align over a launch class's sweeps (classes 1 and 2: st_align<false> and st_align<true> themselves) */
template <int CLS>
__device__ __forceinline__ StAlign sw_align(const uint8_t* qfw, int m, uint8_t* qrv, const uint8_t* ref, int n, int lane, uint8_t* state) {
    if constexpr (CLS == 2) return st_align<true>(qfw, m, qrv, ref, n, lane, state);
    else if constexpr (CLS == 1) return st_align<false>(qfw, m, qrv, ref, n, lane, state);
    else {
        StAlign a{0, 0, -1, 0, -1};
        m = st_uni(m); n = st_uni(n);
        if (m <= 0 || n <= 0) return a;
        const StSweep fw = sw_sweep<0, false>(qfw, m, ref, 0, n, 1, -1, lane, state);
        a.score = fw.score;
        if (fw.score <= 0) return a;
        a.ref_end = fw.col; a.query_end = fw.row;
        const int pm = fw.row + 1;
        for (int x = lane; x < pm; x += 64) qrv[x] = qfw[fw.row - x];
        st_mem_sync();
        const StSweep bw = sw_sweep<0, true>(qrv, pm, ref, fw.col, -1, -1, fw.score, lane, state);
        a.ref_begin = bw.col; a.query_begin = fw.row - bw.row;
        return a;
    }
}

/* one pair on one wave, its buffers in place: align, the indel totals when asked for, the row */
template <int CLS, bool SPAN>
__device__ __forceinline__ void sw_pair(const SwArgs& a, uint32_t s, uint8_t* refc, uint8_t* qfw, uint8_t* qrv, uint32_t qrv_bytes, bool qrv_lds, uint8_t* rows, int8_t* dirbuf, uint8_t* state, int lane) {
    const uint32_t r = st_uni(a.seq_ref[s]);
    const uint32_t m = st_uni(a.b.seq_len[s]), n = st_uni(a.b.seq_len[r]);
    const uint32_t sn = sw_unpack_ref<SPAN>(a, refc, s, r, n, lane);
    sw_unpack(qfw, a.b.bases + a.b.seq_word_off[s], m, lane);
    st_mem_sync();
    const StAlign al = sw_align<CLS>(qfw, (int)m, qrv, refc, (int)sn, lane, state); /* in the span's coordinates, as everything up to the row */
    unsigned ins = 0, del = 0;
    int status = CW_SW_ALIGNED;
    if ((a.flags & CW_SW_WANT_INDELS) && al.score > 0) {
        /* the directions go to the reversed prefix's buffer when it is LDS and they fit, as in the stitch; where they live changes no number */
        if (!st_banded_indels(refc + al.ref_begin, al.ref_end - al.ref_begin + 1, qfw + al.query_begin, al.query_end - al.query_begin + 1, al.score, rows, CW_ST_ROWS_BYTES,
                              dirbuf, a.dir_bytes, &ins, &del, lane, qrv_lds ? (int8_t*)qrv : nullptr, qrv_lds ? qrv_bytes : 0u)) {
            ins = 0; del = 0; status = CW_SW_NO_INDELS;
        }
    }
    if (lane == 0) {
        const int lo = al.score > 0 ? (int)sw_pair_lo<SPAN>(a, s) : 0; /* the row is absolute */
        sw_write_row(a.rows + (size_t)s * CW_SW_ROW, al.score, al.ref_begin + lo, al.ref_end + lo, al.query_begin, al.query_end, ins, del, status);
    }
    st_mem_sync(); /* the next pair's unpacking overwrites what the traceback's lane 0 read */
}

/* a wave's buffers, carved once per launch; refc is chosen per pair */
struct SwWaveBufs {
    uint8_t* ref_lds;    /* CW_ST_RMAX reference codes in the slab; the long launch: none */
    uint8_t* ref_glb;    /* CW_SW_GREF_BYTES of the wave's global scratch */
    uint8_t* refc;       /* the pair's reference: ref_lds or ref_glb */
    uint8_t* qfw;        /* query codes */
    uint8_t* qrv;        /* reversed prefix */
    uint32_t qrv_bytes;  /* what qrv offers the traceback's directions: its size when it is LDS */
    bool qrv_lds;
    uint8_t* rows;       /* CW_ST_ROWS_BYTES of LDS */
    uint8_t* dirbuf;     /* a.dir_bytes of direction scratch; NULL when the run has none */
    uint8_t* steps;      /* CW_SW_STEP_BYTES of step scratch; NULL for the plain run */
    uint8_t* state;      /* the long launch's sweep state */
};

/* The one slab carve and pair-claim loop of classes 0 and 1, for the four runs' kernels: query codes and the reversed prefix in the wave's LDS slab, the
   reference there too up to CW_ST_RMAX bases and in the wave's global scratch beyond.  TRACED: a run with a walk (cw_sw_path.h), which has step scratch at
   steps_base and always has direction scratch; the plain run passes NULL.  per_pair(s, bufs, lane) does one pair (the kernels' lambdas are always_inline, as every device function
   here is: a kernel is one function before the optimiser sees it). */
template <int CLS, bool TRACED, bool SPAN, class F>
__device__ __forceinline__ void sw_class_loop(const SwArgs& a, uint8_t* steps_base, F per_pair) {
    constexpr int QMAX = CLS == 0 ? CW_SW_Q0 : CW_ST_QMAX;
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint8_t* const slab = lds + (size_t)wave * CW_SW_SLAB_OF(QMAX);
    const size_t wv = (size_t)blockIdx.x * CW_SW_WAVES + wave;
    SwWaveBufs w;
    w.ref_lds = slab;                   /* CW_ST_RMAX reference codes */
    w.qfw = w.ref_lds + CW_ST_RMAX;     /* QMAX query codes           */
    w.qrv = w.qfw + QMAX;               /* QMAX reversed prefix       */
    w.rows = w.qrv + QMAX;              /* CW_ST_ROWS_BYTES           */
    w.qrv_bytes = (uint32_t)QMAX; w.qrv_lds = true; w.state = nullptr;
    w.ref_glb = a.gref + wv * CW_SW_GREF_BYTES;
    w.dirbuf = TRACED || a.dir ? (uint8_t*)a.dir + wv * a.dir_bytes : nullptr;
    w.steps = TRACED ? steps_base + wv * CW_SW_STEP_BYTES : nullptr;
    const uint32_t n_pairs = st_uni(a.ctr[3 + CLS]), base = CLS == 0 ? 0u : st_uni(a.ctr[3]);
    for (;;) {
        uint32_t pi = 0;
        if (lane == 0) pi = atomicAdd(a.ctr + CLS, 1u);
        pi = (uint32_t)cw_lane_value((int)pi, 0);
        if (pi >= n_pairs) break;
        const uint32_t s = st_uni(a.order[base + pi]);
        const uint32_t sn = st_uni(sw_pair_len<SPAN>(a, s, a.b.seq_len[st_uni(a.seq_ref[s])]));
        w.refc = sn <= (uint32_t)CW_ST_RMAX ? w.ref_lds : w.ref_glb;
        per_pair(s, w, lane);
    }
}

/* The long class's: one wave a work-group, every buffer and the sweep's state in the wave's global scratch (CW_SW_LONG_WAVE_BYTES); ends at once when the order
   kernel counted no such pair. */
template <bool TRACED, class F>
__device__ __forceinline__ void sw_long_loop(const SwArgs& a, uint8_t* steps_base, F per_pair) {
    __shared__ __attribute__((aligned(16))) uint8_t rows[CW_ST_ROWS_BYTES];
    const int lane = threadIdx.x & 63;
    const uint32_t n_pairs = st_uni(a.ctr[5]);
    if (n_pairs == 0u) return; /* normally */
    const uint32_t base = st_uni(a.ctr[3]) + st_uni(a.ctr[4]);
    SwWaveBufs w;
    w.ref_lds = nullptr;
    w.ref_glb = a.lstate + (size_t)blockIdx.x * CW_SW_LONG_WAVE_BYTES;
    w.refc = w.ref_glb;
    w.qfw = w.refc + CW_SW_GREF_BYTES;
    w.qrv = w.qfw + CW_STH_QMAX;
    w.state = w.qrv + CW_STH_QMAX;
    w.qrv_bytes = 0u; w.qrv_lds = false; w.rows = rows;
    w.dirbuf = TRACED || a.dir ? (uint8_t*)a.dir + (size_t)blockIdx.x * a.dir_bytes : nullptr;
    w.steps = TRACED ? steps_base + (size_t)blockIdx.x * CW_SW_STEP_BYTES : nullptr;
    for (;;) {
        uint32_t pi = 0;
        if (lane == 0) pi = atomicAdd(a.ctr + 2, 1u);
        pi = (uint32_t)cw_lane_value((int)pi, 0);
        if (pi >= n_pairs) break;
        per_pair(st_uni(a.order[base + pi]), w, lane);
    }
}

/* CLS 0: 128 registers (the five-register sweep is its widest: four waves a SIMD, and the LDS of four work-groups a CU); CLS 1: whatever the sixteen-register
   sweep takes (one wave a SIMD, as cw_stitch_kernel's wide instance).  The path, pileup and cut kernels keep these launch bounds. */
template <int CLS, bool SPAN>
__global__ void __launch_bounds__(64 * CW_SW_WAVES, CLS == 0 ? 4 : 1) cw_sw_kernel(SwArgs a) {
    sw_class_loop<CLS, false, SPAN>(a, nullptr, [&](uint32_t s, const SwWaveBufs& w, int lane) __attribute__((always_inline)) {
        sw_pair<CLS, SPAN>(a, s, w.refc, w.qfw, w.qrv, w.qrv_bytes, w.qrv_lds, w.rows, (int8_t*)w.dirbuf, w.state, lane);
    });
}

/* (compiled for 256 registers, two waves a SIMD: at the last launch's 128 of cw_stitch_kernel the memory-state sweep spills 90 registers into its column loop --
   there a launch that normally finds nothing to do, here the path of every long query) */
template <bool SPAN>
__global__ void __launch_bounds__(64, 2) cw_sw_long_kernel(SwArgs a) {
    sw_long_loop<false>(a, nullptr, [&](uint32_t s, const SwWaveBufs& w, int lane) __attribute__((always_inline)) {
        sw_pair<2, SPAN>(a, s, w.refc, w.qfw, w.qrv, w.qrv_bytes, w.qrv_lds, w.rows, (int8_t*)w.dirbuf, w.state, lane);
    });
}

#endif
