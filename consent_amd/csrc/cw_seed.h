/*
 * cw_seed.h -- reads placed on a reference by unique shared k-mers (cw_seed_run / cw_seed_run_device, include/consent_amd.h): per (query, reference) pair whether the
 * query belongs to the reference, on which strand, and on which diagonal -- the strand vote of cw_strand.h with the place of every hit kept.
 *
 * The shape is cw_strand.h's: cw_strand_units_kernel is launched as it is (it reads the batch, unit_off and ctr only), the two launch classes, the chunks of
 * CW_STR_CHUNK / CW_STR_CHUNK_WIDE queries and the claim loop are its.  What differs is the table and what a hit does:
 *
 *   the table    a slot is one 32-bit word: a reference POSITION (<= CW_SW_RMAX, 14 bits), bit 31 "this k-mer occurs more than once", 0xFFFFFFFF empty.  The
 *                reference's packed words are staged in LDS beside the table (4 KB at 16 383 bases), and the key of a slot is the k-mer cut from them at the
 *                slot's position (cw_kmer_at): membership stays exact, and positions cost no second 128 KB array.  Insert: compare-and-swap empty -> j; on a
 *                slot that is taken, compare the k-mer at its position with the key -- equal: OR the flag in and stop (whose position stays is then of no
 *                interest: a flagged slot seeds nothing), else probe on.  A lookup gives the position only when the flag is clear: repeats and homopolymer
 *                runs do not vote.  Linear probing behind cw_strand.h's hash, at most half full.
 *   a hit        position i of the query as given, on reference position p: diagonal d = p - i, bin (d + m) >> CW_SEED_SHIFT.  Its reverse complement on p: that
 *                is position m - k - i of the turned query, so the bin is (p + k + i) >> CW_SEED_SHIFT -- no turned query is made.  A wave owns two histograms
 *                (forward, reverse) of 16-bit counts, two to a word, added with LDS atomicAdd(1 << 16 (b & 1)): a count is at most m - k + 1 < 65 536.
 *   the row      the lanes over the bins b: w[b] = c[b] + c[b + 1], a window of 128 diagonals; per orientation the wave's maximum of w << 10 | (1023 - b) -- the
 *                largest w, then the lowest b -- and lane 0 stores STATUS, HITS, DIAG = (b << 6) - m, OTHER with plain stores: reverse only when its best w is
 *                the larger.
 *
 * cw_seed_spans_kernel (cw_seed_spans / cw_seed_spans_device) turns the rows into the reference spans the aligner's span runs take: one thread a sequence.
 *
 * LDS.  WIDE = 0 (references of up to CW_ST_RMAX = 2 048 bases): 16 KB table + 512 B words + 4 waves x 2 x 273 words of histogram (B <= 545 bins and the
 * zero bin behind them) = 25 632 B static, 256 threads, six work-groups a CU.  WIDE = 1 (up to CW_SW_RMAX): 128 KB table + 4 KB words + 8 waves x 2 x 385
 * words (B <= 768) = 159 808 B dynamic, 512 threads, one work-group a CU.
 *
 * Waves of a work-group take different numbers of queries: inside the per-query loop there is no __syncthreads(), only cw_wave_sync() between a histogram's
 * clear, its atomics and its scan.  Probe loops end because a table is at most half full.  No inline assembly, plain C++ stores only, no environment switch.
 */
#ifndef CW_SEED_H
#define CW_SEED_H

#include "cw_strand.h"

#define CW_SEED_THREADS_WIDE 512
#define CW_SEED_REPEAT 0x80000000u /* a slot's flag: its k-mer occurs at more than one position */
#define CW_SEED_POS 0x3FFFu        /* a slot's position */
#define CW_SEED_NO_HIT 0xFFFFFFFFu /* what a lookup gives for a k-mer that is absent or repeated */
/* the words of a staged reference, and of one histogram: bins 0 .. B - 1 with B = ((n + m) >> CW_SEED_SHIFT) + 1 and the zero bin B, two a word */
#define CW_SEED_RWORDS(rmax) (((rmax) + 15u) / 16u)
#define CW_SEED_HWORDS(rmax) (((((rmax) + (uint32_t)CW_SW_QMAX) >> CW_SEED_SHIFT) + 3u) / 2u)
#define CW_SEED_LDS_WORDS(slots, rmax, threads) ((slots) + CW_SEED_RWORDS(rmax) + ((threads) / 64u) * 2u * CW_SEED_HWORDS(rmax))

static_assert(2u * CW_ST_RMAX <= CW_STR_SLOTS && 2u * CW_SW_RMAX <= CW_STR_SLOTS_WIDE, "a table is at most half full: every probe loop meets an empty slot");
static_assert(CW_SW_RMAX <= CW_SEED_POS && (CW_STR_EMPTY & CW_SEED_REPEAT), "a position fits a slot beside the flag, and an empty slot is none");
static_assert(CW_SW_QMAX < 65536u, "a 16-bit count holds the positions of a query");
static_assert((((uint32_t)CW_SW_RMAX + (uint32_t)CW_SW_QMAX) >> CW_SEED_SHIFT) + 1u <= 1023u, "a bin fits the ten low bits of the scan's key, its count the bits above");
static_assert(CW_SEED_LDS_WORDS(CW_STR_SLOTS, CW_ST_RMAX, CW_STR_THREADS) * 4u * 6u <= 160u * 1024u, "cw_seed_kernel<0>: six work-groups a CU");
static_assert(CW_SEED_LDS_WORDS(CW_STR_SLOTS_WIDE, CW_SW_RMAX, CW_SEED_THREADS_WIDE) * 4u <= 160u * 1024u - 1024u, "cw_seed_kernel<1>: the table, the words, the histograms and the claimed unit in a work-group's LDS");

struct SeedArgs {
    DevBatch b;
    uint32_t n_seqs;
    int32_t* rows;            /* [n_seqs * CW_SEED_ROW], the caller's */
    uint8_t* strand;          /* [n_seqs] or NULL */
    uint32_t k;               /* CW_STRAND_KMIN .. CW_STRAND_KMAX */
    const uint32_t* unit_off; /* [n_windows + 1] scratch, cw_strand_units_kernel's */
    uint32_t* ctr;            /* CW_STR_CTR_WORDS scratch: [0], [1] zero before the seed launches, [2], [3] the units kernel's */
};

__device__ __forceinline__ void seed_store(const SeedArgs& a, uint32_t s, uint32_t status, uint32_t hits, int32_t diag, uint32_t other) {
    int32_t* const row = a.rows + (size_t)s * CW_SEED_ROW;
    row[CW_SEED_STATUS] = (int32_t)status; row[CW_SEED_HITS] = (int32_t)hits; row[CW_SEED_DIAG] = diag; row[CW_SEED_OTHER] = (int32_t)other;
    if (a.strand) a.strand[s] = (uint8_t)status;
}

/* the one position of key in the reference, or CW_SEED_NO_HIT: the slots from its hash on hold the position of this k-mer, or of another, until an empty one */
template <uint32_t SLOTS, uint32_t BITS>
__device__ __forceinline__ uint32_t seed_find(const uint32_t* tab, const uint32_t* rw, uint32_t key, uint32_t k) {
    uint32_t h = strand_hash(key, BITS);
    for (;;) {
        const uint32_t v = tab[h];
        if (v == CW_STR_EMPTY) return CW_SEED_NO_HIT;
        if (cw_kmer_at(rw, v & CW_SEED_POS, k) == key) return (v & CW_SEED_REPEAT) ? CW_SEED_NO_HIT : v;
        h = (h + 1u) & (SLOTS - 1u);
    }
}

__device__ __forceinline__ void seed_count(uint32_t* hist, uint32_t bin) { atomicAdd(&hist[bin >> 1], 1u << (16u * (bin & 1u))); }
__device__ __forceinline__ uint32_t seed_bin(const uint32_t* hist, uint32_t bin) { return (hist[bin >> 1] >> (16u * (bin & 1u))) & 0xFFFFu; }

/* cw_seed_spans_device: the reference columns a placed query can reach, for the span runs of the aligner (cw_sw_span_run and its kin).  One thread per sequence,
   its group by bisection as the order kernel finds it; 64-bit signed arithmetic, so no DIAG, pad or shift overflows.  A row that places nothing -- a reference's
   own, CW_STRAND_NONE, fewer than min_hits -- gives the empty span (0, 0). */
struct SeedSpanArgs {
    DevBatch b;
    uint32_t n_seqs;
    const int32_t* rows;      /* [n_seqs * CW_SEED_ROW], a seed run's */
    uint32_t min_hits, pad, pad_shift;
    uint32_t* ref_lo;         /* [n_seqs] */
    uint32_t* ref_hi;
};

__global__ void __launch_bounds__(256) cw_seed_spans_kernel(SeedSpanArgs a) {
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    if (s >= a.n_seqs) return;
    uint32_t lo = 0, hi = a.b.n_windows; /* win_first_seq[lo] <= s < win_first_seq[hi] */
    while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (a.b.win_first_seq[mid] <= s) lo = mid; else hi = mid; }
    const int32_t* const row = a.rows + (size_t)s * CW_SEED_ROW;
    const int64_t n = (int64_t)a.b.seq_len[a.b.win_first_seq[lo]], m = (int64_t)a.b.seq_len[s];
    const int32_t status = row[CW_SEED_STATUS];
    int64_t c0 = 0, c1 = 0;
    if ((status == CW_STRAND_FWD || status == CW_STRAND_REV) && (int64_t)row[CW_SEED_HITS] >= (int64_t)a.min_hits) {
        const int64_t P = (int64_t)a.pad + (m >> a.pad_shift), d = (int64_t)row[CW_SEED_DIAG];
        c0 = d - P; c1 = d + (int64_t)(2u << CW_SEED_SHIFT) + m + P;
        c0 = c0 < 0 ? 0 : c0 > n ? n : c0;
        c1 = c1 < 0 ? 0 : c1 > n ? n : c1;
    }
    a.ref_lo[s] = (uint32_t)c0; a.ref_hi[s] = (uint32_t)c1;
}

template <int WIDE>
__global__ void __launch_bounds__(WIDE ? CW_SEED_THREADS_WIDE : CW_STR_THREADS) cw_seed_kernel(SeedArgs a) {
    constexpr uint32_t SLOTS = WIDE ? CW_STR_SLOTS_WIDE : CW_STR_SLOTS, BITS = WIDE ? 15u : 12u, THREADS = WIDE ? CW_SEED_THREADS_WIDE : CW_STR_THREADS;
    constexpr uint32_t RMAX = WIDE ? (uint32_t)CW_SW_RMAX : (uint32_t)CW_ST_RMAX, RWORDS = CW_SEED_RWORDS(RMAX), HWORDS = CW_SEED_HWORDS(RMAX);
    static_assert((1u << BITS) == SLOTS, "the hash gives a slot");
    extern __shared__ uint32_t seed_dyn[];
    __shared__ uint32_t lds_static[WIDE ? 1 : CW_SEED_LDS_WORDS(SLOTS, RMAX, THREADS)];
    __shared__ uint32_t claimed;
    if (a.ctr[2 + WIDE] == 0u) return; /* no group of this class */
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, k = a.k;
    uint32_t* const tab = WIDE ? seed_dyn : lds_static;
    uint32_t* const rw = tab + SLOTS;                           /* the reference's packed words */
    uint32_t* const fwd = rw + RWORDS + wave * 2u * HWORDS;     /* this wave's histograms */
    uint32_t* const rev = fwd + HWORDS;
    const uint32_t n_units = a.unit_off[a.b.n_windows];
    for (;;) {
        __syncthreads(); /* the unit before is done with the table, the words and with `claimed` */
        if (tid == 0) claimed = atomicAdd(&a.ctr[WIDE], 1u);
        __syncthreads();
        const uint32_t u = claimed;
        if (u >= n_units) break;
        uint32_t lo = 0, hi = a.b.n_windows; /* the group of u: the last with unit_off[g] <= u (cw_strand_kernel) */
        while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (a.unit_off[mid] <= u) lo = mid; else hi = mid; }
        const uint32_t r = a.b.win_first_seq[lo], q_end = a.b.win_first_seq[lo + 1];
        const uint32_t n = a.b.seq_len[r];
        if (strand_class(n) != (uint32_t)WIDE) continue; /* the other launch's */
        const uint32_t c = u - a.unit_off[lo], chunk = strand_chunk(n);
        const uint32_t s0 = r + 1u + c * chunk, s1 = q_end - s0 > chunk ? s0 + chunk : q_end;
        if (c == 0u && tid == 0u) seed_store(a, r, CW_STRAND_IS_REF, 0u, 0, 0u);
        if (n < k || n > (uint32_t)CW_SW_RMAX) { /* no vote against this reference */
            for (uint32_t s = s0 + tid; s < s1; s += THREADS) seed_store(a, s, CW_STRAND_NONE, 0u, 0, 0u);
            continue;
        }
        const uint32_t* const gw = a.b.bases + a.b.seq_word_off[r];
        for (uint32_t x = tid; x < SLOTS; x += THREADS) tab[x] = CW_STR_EMPTY;
        for (uint32_t x = tid; x < (n + 15u) / 16u; x += THREADS) rw[x] = gw[x]; /* (n <= RMAX of this class: at most RWORDS) */
        __syncthreads();
        for (uint32_t j = tid; j + k <= n; j += THREADS) {
            const uint32_t key = cw_kmer_at(rw, j, k);
            uint32_t h = strand_hash(key, BITS);
            for (;;) {
                const uint32_t old = atomicCAS(&tab[h], CW_STR_EMPTY, j);
                if (old == CW_STR_EMPTY) break;
                if (cw_kmer_at(rw, old & CW_SEED_POS, k) == key) { atomicOr(&tab[h], CW_SEED_REPEAT); break; }
                h = (h + 1u) & (SLOTS - 1u);
            }
        }
        __syncthreads();
        for (uint32_t s = s0 + wave; s < s1; s += THREADS / 64u) { /* a query a wave, the lanes over its positions; no work-group barrier in here */
            const uint32_t m = a.b.seq_len[s];
            if (m < k || m > (uint32_t)CW_SW_QMAX) { if (lane == 0u) seed_store(a, s, CW_STRAND_NONE, 0u, 0, 0u); continue; }
            const uint32_t B = ((n + m) >> CW_SEED_SHIFT) + 1u; /* bins 0 .. B - 1, and bin B that stays zero: (B + 2) / 2 <= HWORDS words */
            cw_wave_sync(); /* the query before is scanned */
            for (uint32_t x = lane; x < (B + 2u) / 2u; x += 64u) { fwd[x] = 0u; rev[x] = 0u; }
            cw_wave_sync();
            const uint32_t* const qw = a.b.bases + a.b.seq_word_off[s];
            for (uint32_t i = lane; i + k <= m; i += 64u) {
                const uint32_t key = cw_kmer_at(qw, i, k);
                const uint32_t p = seed_find<SLOTS, BITS>(tab, rw, key, k);
                if (p != CW_SEED_NO_HIT) seed_count(fwd, (p + m - i) >> CW_SEED_SHIFT);      /* d + m, d = p - i */
                const uint32_t t = seed_find<SLOTS, BITS>(tab, rw, strand_rc(key, k), k);
                if (t != CW_SEED_NO_HIT) seed_count(rev, (t + k + i) >> CW_SEED_SHIFT);      /* d + m, d = t - (m - k - i) */
            }
            cw_wave_sync();
            int best_f = 0, best_r = 0; /* w << 10 | (1023 - b): the largest w, then the lowest b */
            for (uint32_t b = lane; b < B; b += 64u) {
                best_f = max(best_f, (int)(((seed_bin(fwd, b) + seed_bin(fwd, b + 1u)) << 10) | (1023u - b)));
                best_r = max(best_r, (int)(((seed_bin(rev, b) + seed_bin(rev, b + 1u)) << 10) | (1023u - b)));
            }
            const uint32_t kf = (uint32_t)cw_wave_max(best_f), kr = (uint32_t)cw_wave_max(best_r); /* (lane 0 has bin 0: a key is at least 1023 - 0) */
            if (lane == 0u) {
                const uint32_t wf = kf >> 10, wr = kr >> 10;
                if (wr > wf) seed_store(a, s, CW_STRAND_REV, wr, (int32_t)((1023u - (kr & 1023u)) << CW_SEED_SHIFT) - (int32_t)m, wf);
                else seed_store(a, s, CW_STRAND_FWD, wf, (int32_t)((1023u - (kf & 1023u)) << CW_SEED_SHIFT) - (int32_t)m, wr);
            }
        }
    }
}

#endif
