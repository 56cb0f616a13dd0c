/*
 * cw_locate.h -- reads placed on a reference of any length through ONE index of the whole reference's unique k-mers (cw_locate_build_device, cw_locate_run_device,
 * cw_locate_run, include/consent_amd.h): cw_seed.h's design moved to global memory.  A read costs O(m) whatever the reference's length.
 *
 *   the index    "positions, not keys" again.  A slot of the caller's table is one 32-bit word: a reference POSITION (<= CW_LOCATE_RMAX, 28 bits), bit 31 "this
 *                k-mer occurs more than once", 0xFFFFFFFF empty; bits 28 - 30 are zero.  A slot's key is the k-mer cut from the reference's own words at that
 *                position (cw_kmer_at on the global reference): membership stays exact and no key array exists.  The build is a clear and one thread per
 *                position: compare-and-swap empty -> j; on a slot that is taken, compare the k-mer at its position with the key -- equal: OR the flag in and
 *                stop, else probe on.  A lookup gives the position only when the flag is clear.  Linear probing behind cw_strand.h's hash at the table's
 *                width; the table has at least twice the reference's positions (cw_locate_table_words), so every probe loop meets an empty slot.
 *   the votes    a SPARSE histogram: the bins of a long reference run to millions, the distinct (orientation, bin) pairs of a read are at most its hits.  One
 *                work-group takes one read at a time -- claimed through an atomicAdd counter, in the order given -- with its threads over the read's positions,
 *                and counts into an open-addressing table of its own: a key array with compare-and-swap empty -> (o << 31 | b), beside it 16-bit counts, two
 *                to a word, added as seed_count adds them (a count is at most m - k + 1 < 65 536).
 *   the row      the threads over the slots: an occupied slot (o, b, c) proposes window b, c + count(o, b + 1), and, when b >= 1, window b - 1,
 *                count(o, b - 1) + c.  Every window with a hit has an occupied bin, so these are all of them; per orientation the work-group's maximum of
 *                w << 32 | ~b -- the largest w, then the lowest b -- starts from w = 0 at bin 0, the row of a read without a hit.  Thread 0 stores STATUS, HITS,
 *                DIAG = (b << 6) - m, OTHER with plain stores: reverse only when its best w is the larger.
 *   two routes   cw_locate_kernel<0>: the sparse table in LDS, CW_LOC_SLOTS = 4 096 keys + 2 048 count words = 24 KB, 256 threads, six work-groups a CU -- the
 *                kernel is made of dependent global gathers, and waves are what hides them.  A read whose distinct pairs pass CW_LOC_CAP = half the table is
 *                abandoned and its index appended to a redo list in scratch: a thread looks at the count before each position, so at most two inserts a
 *                thread land beyond the capacity and the table never fills.  cw_locate_kernel<1>, a second launch over that list, is the same code with the
 *                table in global scratch, one per work-group of the launch: a read clears and uses the power of two that holds 4 (m - k + 1) slots -- its
 *                pairs are at most 2 (m - k + 1), half of that.  The route is a function of the read's distinct pairs alone, and both compute the same row.
 *
 * No inline assembly, plain C++ stores only, no environment switch.
 */
#ifndef CW_LOCATE_H
#define CW_LOCATE_H

#include "cw_seed.h"

#define CW_LOC_THREADS 256
#define CW_LOC_SLOTS 4096u                  /* the LDS route's sparse table */
#define CW_LOC_BITS 12u
#define CW_LOC_CAP (CW_LOC_SLOTS / 2u)      /* the distinct pairs it takes */
#define CW_LOC_DENSE_BITS 17u               /* the dense route's table: 4 (m - k + 1) <= 4 CW_SW_QMAX slots */
#define CW_LOC_DENSE_SLOTS (1u << CW_LOC_DENSE_BITS)
#define CW_LOC_DENSE_WORDS (CW_LOC_DENSE_SLOTS + CW_LOC_DENSE_SLOTS / 2u) /* keys, and counts two to a word */
#define CW_LOC_POS 0x0FFFFFFFu              /* a slot's position */
#define CW_LOC_TABLE_MIN 1024u              /* the smallest table */
#define CW_LOC_CTR_WORDS 8u                 /* [0]: the LDS launch's claim counter; [1]: the redo list's length; [2]: the dense launch's claim counter */

static_assert((1u << CW_LOC_BITS) == CW_LOC_SLOTS, "the hash gives a slot");
static_assert(CW_LOC_CAP + 2u * CW_LOC_THREADS < CW_LOC_SLOTS, "the LDS route: each thread inserts at most two pairs after it saw the count within the capacity, so a slot stays empty and every probe loop ends");
static_assert(4u * (uint32_t)CW_SW_QMAX <= CW_LOC_DENSE_SLOTS, "the dense route: 2 (m - k + 1) pairs at most in 4 (m - k + 1) slots or more, at most half full");
static_assert(CW_LOCATE_RMAX <= CW_LOC_POS && (CW_STR_EMPTY & CW_SEED_REPEAT) && (CW_STR_EMPTY & ~(CW_LOC_POS | CW_SEED_REPEAT)), "a position fits a slot beside the flag, and no slot in use is the empty word");
static_assert((((uint64_t)CW_LOCATE_RMAX + (uint64_t)CW_SW_QMAX) >> CW_SEED_SHIFT) < 0x7FFFFFFFull, "a bin fits the 31 low bits of a pair, and no pair is the empty word");
static_assert((uint64_t)CW_LOCATE_RMAX + (uint64_t)CW_SW_QMAX < 0x80000000ull, "DIAG fits an int32");
static_assert((CW_LOC_SLOTS + CW_LOC_SLOTS / 2u) * 4u * 6u <= 160u * 1024u - 6u * 64u, "cw_locate_kernel<0>: six work-groups a CU");

/* the words of a table for a reference of n bases: a power of two, at least twice the positions (host and device) */
__host__ __device__ inline uint32_t cw_loc_table_bits(uint64_t n) {
    uint32_t bits = 10u;
    while (((uint64_t)1 << bits) < 2u * n) ++bits;
    return bits;
}
static_assert((1u << 10) == CW_LOC_TABLE_MIN, "cw_loc_table_bits' floor");

struct LocateRefArgs {
    const uint32_t* ref; /* the reference's packed words */
    uint32_t n;          /* <= CW_LOCATE_RMAX */
    uint32_t* table;     /* [1 << bits], the caller's */
    uint32_t bits;       /* cw_loc_table_bits(n): 10 .. 29 */
    uint32_t k;          /* CW_STRAND_KMIN .. CW_STRAND_KMAX */
};

struct LocateArgs {
    LocateRefArgs r;
    uint32_t n_seqs;
    const uint32_t* seq_len;      /* the reads: their grouping is not read */
    const uint64_t* seq_word_off;
    const uint32_t* bases;
    int32_t* rows;                /* [n_seqs * CW_SEED_ROW], the caller's */
    uint8_t* strand;              /* [n_seqs] or NULL */
    uint32_t* ctr;                /* CW_LOC_CTR_WORDS scratch, zero before the run */
    uint32_t* redo;               /* [n_seqs] scratch: the reads the LDS route abandoned */
    uint32_t* dense;              /* [dense work-groups * CW_LOC_DENSE_WORDS] scratch */
    uint32_t* routes;             /* [2], the engine's: reads of the LDS route, reads of the dense route (cw_debug_locate_routes) */
};

/* one thread per position of the reference; the table is cleared before */
__global__ void __launch_bounds__(256) cw_locate_build_kernel(LocateRefArgs a) {
    const uint32_t k = a.k, mask = (1u << a.bits) - 1u;
    if (a.n < k) return;
    const uint32_t last = a.n - k; /* the last position */
    for (uint64_t j64 = (uint64_t)blockIdx.x * 256u + threadIdx.x; j64 <= last; j64 += (uint64_t)gridDim.x * 256u) {
        const uint32_t j = (uint32_t)j64, key = cw_kmer_at(a.ref, j, k);
        uint32_t h = strand_hash(key, a.bits);
        for (;;) {
            const uint32_t old = atomicCAS(&a.table[h], CW_STR_EMPTY, j);
            if (old == CW_STR_EMPTY) break;
            if (cw_kmer_at(a.ref, old & CW_LOC_POS, k) == key) { atomicOr(&a.table[h], CW_SEED_REPEAT); break; }
            h = (h + 1u) & mask;
        }
    }
}

/* the one position of key in the reference, or CW_SEED_NO_HIT (seed_find on the global table) */
__device__ __forceinline__ uint32_t locate_find(const LocateRefArgs& r, uint32_t key) {
    const uint32_t mask = (1u << r.bits) - 1u;
    uint32_t h = strand_hash(key, r.bits);
    for (;;) {
        const uint32_t v = r.table[h];
        if (v == CW_STR_EMPTY) return CW_SEED_NO_HIT;
        if (cw_kmer_at(r.ref, v & CW_LOC_POS, r.k) == key) return (v & CW_SEED_REPEAT) ? CW_SEED_NO_HIT : v;
        h = (h + 1u) & mask;
    }
}

/* one hit of the pair (o << 31 | b) into the sparse table; a pair's first hit counts in *distinct */
__device__ __forceinline__ void locate_count(uint32_t* keys, uint32_t* cnt, uint32_t bits, uint32_t pair, uint32_t* distinct) {
    const uint32_t mask = (1u << bits) - 1u;
    uint32_t h = strand_hash(pair, bits);
    for (;;) {
        const uint32_t old = atomicCAS(&keys[h], CW_STR_EMPTY, pair);
        if (old == CW_STR_EMPTY) atomicAdd(distinct, 1u);
        if (old == CW_STR_EMPTY || old == pair) { atomicAdd(&cnt[h >> 1], 1u << (16u * (h & 1u))); return; }
        h = (h + 1u) & mask;
    }
}

/* the count of a pair, 0 when it has no slot */
__device__ __forceinline__ uint32_t locate_count_of(const uint32_t* keys, const uint32_t* cnt, uint32_t bits, uint32_t pair) {
    const uint32_t mask = (1u << bits) - 1u;
    uint32_t h = strand_hash(pair, bits);
    for (;;) {
        const uint32_t v = keys[h];
        if (v == CW_STR_EMPTY) return 0u;
        if (v == pair) return (cnt[h >> 1] >> (16u * (h & 1u))) & 0xFFFFu;
        h = (h + 1u) & mask;
    }
}

__device__ __forceinline__ void locate_store(const LocateArgs& a, uint32_t s, uint32_t status, uint32_t hits, int32_t diag, uint32_t other) {
    int32_t* const row = a.rows + (size_t)s * CW_SEED_ROW;
    row[CW_SEED_STATUS] = (int32_t)status; row[CW_SEED_HITS] = (int32_t)hits; row[CW_SEED_DIAG] = diag; row[CW_SEED_OTHER] = (int32_t)other;
    if (a.strand) a.strand[s] = (uint8_t)status;
}

/* DENSE = 0: every read, the sparse table in LDS.  DENSE = 1: the reads of the redo list, the table in this work-group's piece of a.dense. */
template <int DENSE>
__global__ void __launch_bounds__(CW_LOC_THREADS) cw_locate_kernel(LocateArgs a) {
    __shared__ uint32_t lds_tab[DENSE ? 1 : CW_LOC_SLOTS + CW_LOC_SLOTS / 2u];
    __shared__ unsigned long long best[2]; /* per orientation w << 32 | ~b */
    __shared__ uint32_t claimed, distinct;
    const uint32_t tid = threadIdx.x, k = a.r.k, n = a.r.n;
    const uint32_t n_todo = DENSE ? a.ctr[1] : a.n_seqs;
    if (DENSE && blockIdx.x == 0u && tid == 0u) { a.routes[0] = a.n_seqs - n_todo; a.routes[1] = n_todo; }
    uint32_t* const base = DENSE ? a.dense + (size_t)blockIdx.x * CW_LOC_DENSE_WORDS : lds_tab;
    for (;;) {
        __syncthreads(); /* the read before is done with the table, `best` and `claimed` */
        if (tid == 0) claimed = atomicAdd(&a.ctr[DENSE ? 2 : 0], 1u);
        __syncthreads();
        if (claimed >= n_todo) break;
        const uint32_t s = DENSE ? a.redo[claimed] : claimed;
        const uint32_t m = a.seq_len[s];
        if (m < k || m > (uint32_t)CW_SW_QMAX || n < k) { if (tid == 0) locate_store(a, s, CW_STRAND_NONE, 0u, 0, 0u); continue; }
        uint32_t bits = CW_LOC_BITS; /* DENSE: the power of two that holds 4 (m - k + 1) slots */
        if (DENSE) { bits = 6u; while ((1u << bits) < 4u * (m - k + 1u)) ++bits; }
        const uint32_t slots = 1u << bits;
        uint32_t* const keys = base;
        uint32_t* const cnt = base + slots;
        for (uint32_t x = tid; x < slots; x += CW_LOC_THREADS) keys[x] = CW_STR_EMPTY;
        for (uint32_t x = tid; x < slots / 2u; x += CW_LOC_THREADS) cnt[x] = 0u;
        if (tid == 0) { distinct = 0u; best[0] = 0xFFFFFFFFull; best[1] = 0xFFFFFFFFull; } /* w = 0 at bin 0 */
        if (DENSE) __threadfence(); /* the cleared words are in L2, where the other waves' atomics find them */
        __syncthreads();
        const uint32_t* const qw = a.bases + a.seq_word_off[s];
        for (uint32_t i = tid; i + k <= m; i += CW_LOC_THREADS) {
            if (!DENSE && *(volatile uint32_t*)&distinct > CW_LOC_CAP) break; /* abandoned: at most two more pairs a thread came in behind this look */
            const uint32_t key = cw_kmer_at(qw, i, k);
            const uint32_t p = locate_find(a.r, key);
            if (p != CW_SEED_NO_HIT) locate_count(keys, cnt, bits, (p + m - i) >> CW_SEED_SHIFT, &distinct);                 /* d + m, d = p - i */
            const uint32_t t = locate_find(a.r, strand_rc(key, k));
            if (t != CW_SEED_NO_HIT) locate_count(keys, cnt, bits, 0x80000000u | ((t + k + i) >> CW_SEED_SHIFT), &distinct); /* d + m, d = t - (m - k - i) */
        }
        __syncthreads();
        if (DENSE) __threadfence(); /* the atomics ran in L2: no line of the table this CU loaded before them is read below */
        if (!DENSE && distinct > CW_LOC_CAP) { /* (the count only grows: the same answer in every thread) */
            if (tid == 0) a.redo[atomicAdd(&a.ctr[1], 1u)] = s;
            continue;
        }
        unsigned long long mine[2] = {0ull, 0ull};
        for (uint32_t x = tid; x < slots; x += CW_LOC_THREADS) {
            const uint32_t pair = keys[x];
            if (pair == CW_STR_EMPTY) continue;
            const uint32_t o = pair >> 31, b = pair & 0x7FFFFFFFu, c = (cnt[x >> 1] >> (16u * (x & 1u))) & 0xFFFFu;
            const unsigned long long up = ((unsigned long long)(c + locate_count_of(keys, cnt, bits, pair + 1u)) << 32) | (0xFFFFFFFFu - b);
            mine[o] = up > mine[o] ? up : mine[o];
            if (b >= 1u) {
                const unsigned long long down = ((unsigned long long)(locate_count_of(keys, cnt, bits, pair - 1u) + c) << 32) | (0xFFFFFFFFu - (b - 1u));
                mine[o] = down > mine[o] ? down : mine[o];
            }
        }
        if (mine[0]) atomicMax(&best[0], mine[0]);
        if (mine[1]) atomicMax(&best[1], mine[1]);
        __syncthreads();
        if (tid == 0) {
            const uint32_t wf = (uint32_t)(best[0] >> 32), wr = (uint32_t)(best[1] >> 32);
            const uint32_t bf = 0xFFFFFFFFu - (uint32_t)best[0], br = 0xFFFFFFFFu - (uint32_t)best[1];
            if (wr > wf) locate_store(a, s, CW_STRAND_REV, wr, (int32_t)(br << CW_SEED_SHIFT) - (int32_t)m, wf);
            else locate_store(a, s, CW_STRAND_FWD, wf, (int32_t)(bf << CW_SEED_SHIFT) - (int32_t)m, wr);
        }
    }
}

#endif
