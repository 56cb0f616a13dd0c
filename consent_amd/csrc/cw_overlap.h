/*
 * cw_overlap.h -- the reads of a set that overlap each other, through ONE index that keeps EVERY occurrence of a sampled canonical k-mer (cw_overlap_count_device,
 * cw_overlap_build_device, cw_overlap_run_device, cw_overlap_run, cw_overlap_to_pile_device, include/consent_amd.h): cw_locate.h's vote keyed by target read.
 *
 *   the index    the caller's memory: CW_OVL_HDR words, then three arrays of S slots -- S a power of two, at least twice the entries, at most 2^31 (a key is
 *                below 2^30) -- and the postings, one 64-bit word each (read | position << 24 | strand << 40).  keys[h] is a canonical k-mer or CW_STR_EMPTY,
 *                cnt[h] its occurrences, off[h] the END of its postings.  Four passes over the reads, a work-group a read, threads over its positions:
 *                  count    the sampled positions, summed into the header -- the caller's n_entries is held against it: when they differ no later pass does
 *                           anything, the header keeps CW_OVL_MAGIC out, and a run against that memory answers CW_OVL_BAD_INDEX for every query
 *                  insert   compare-and-swap empty -> c behind ovl_hash, linear probing, then an atomic add into cnt[h]
 *                  assign   a thread a slot: a work-group's counts are scanned in LDS and ONE atomic add on the header's cursor gives it its piece of the
 *                           postings; off[h] = where the slot's begin.  (No scan over all slots: the order of the keys' pieces is private, as the order inside.)
 *                  fill     postings[atomicAdd(&off[h], 1)] = the position's word; afterwards off[h] is the end and off[h] - cnt[h] the beginning
 *                The sample's own hash takes the TOP bits of c * 0x9E3779B1 to be zero, so the table hashes with another multiplier (ovl_hash): strand_hash
 *                would put every sampled key into the first 2^-sample of the slots.
 *   the votes    one work-group takes one query at a time through a counter; its threads run over the query's positions, a thread over the postings of its
 *                hit (occ <= max_occ read from cnt[h]).  A vote is the 36-bit key t << 12 | o << 11 | b in a 64-bit word, counted in an open-addressing table:
 *                64-bit compare-and-swap empty -> key, beside it a 32-bit count.  A count is at most 64 (m - k + 1): for one position the postings of one target
 *                that fall into one bin are 64 diagonals, so 32 bits never wrap and a window's w is below 2^22 (static_assert below).
 *   the windows  threads over the occupied slots: slot (t, o, b, c) proposes windows b and b - 1 as cw_locate_kernel does, and the maximum of w << 32 | ~b goes
 *                into a second table keyed t << 1 | o (64-bit atomicMax).  Its slots with w >= min_hits are the candidates; each becomes one 64-bit word
 *                (0x3FFFFF - w) << 36 | t << 12 | o << 11 | b in a list that reuses the first table's keys, and a candidate's rank is the number of smaller
 *                words: hits descending, then t, then o.  Rank r writes row r with plain stores; a slot too small gets the count and CW_OVL_SLOT, no row.
 *   two routes   cw_overlap_kernel<0>: both tables in LDS, CW_OVL_SLOTS = 2 048 slots each, 48 KB, 256 threads, three work-groups a CU.  A query whose distinct
 *                keys pass CW_OVL_CAP = half the table is abandoned and appended to a redo list: a thread looks at the count before EACH vote, so at most
 *                one insert a thread lands beyond the capacity.  cw_overlap_kernel<1>, a second launch over the list: the same code, the tables in this
 *                work-group's piece of scratch, CW_OVL_DENSE_SLOTS = 2^18 slots each.  A query whose distinct keys pass CW_OVL_DENSE_CAP = 2^17 even there is
 *                CW_OVL_DENSE: no rows.  Both thresholds compare the number of distinct (t, o, b) keys, a function of the set, the parameters and the query.
 *
 * No inline assembly, plain C++ stores only, no environment switch.
 */
#ifndef CW_OVERLAP_H
#define CW_OVERLAP_H

#include "cw_locate.h"

#define CW_OVL_THREADS 256
#define CW_OVL_BITS 11u
#define CW_OVL_SLOTS 2048u                       /* the LDS route's two tables */
#define CW_OVL_CAP (CW_OVL_SLOTS / 2u)           /* the distinct keys it takes */
#define CW_OVL_DENSE_BITS 18u
#define CW_OVL_DENSE_SLOTS (1u << CW_OVL_DENSE_BITS)
#define CW_OVL_DENSE_CAP (CW_OVL_DENSE_SLOTS / 2u)
#define CW_OVL_TABLE_WORDS(slots) (6u * (slots)) /* keys 2, counts 1; the second table: keys 1, values 2 */
#define CW_OVL_DENSE_WORDS CW_OVL_TABLE_WORDS(CW_OVL_DENSE_SLOTS)
#define CW_OVL_HDR 16u                           /* [0] CW_OVL_MAGIC once built; [2..3] the counted entries; [4] the postings' cursor */
#define CW_OVL_MAGIC 0x4F564C31u
#define CW_OVL_TABLE_MIN 1024u
#define CW_OVL_CTR_WORDS 8u                      /* as CW_LOC_CTR_WORDS: [0] the LDS launch's claim counter; [1] the redo list's length; [2] the dense launch's */
#define CW_OVL_EMPTY64 0xFFFFFFFFFFFFFFFFull
#define CW_OVL_READS_MAX ((1u << 24) - 1u)
#define CW_OVL_MAX_OCC_MAX 65535u
#define CW_OVL_SAMPLE_MAX 8u

static_assert((1u << CW_OVL_BITS) == CW_OVL_SLOTS, "the hash gives a slot");
static_assert(CW_OVL_CAP + CW_OVL_THREADS < CW_OVL_SLOTS, "the LDS route: a thread inserts at most one key after it saw the count within the capacity, so a slot stays empty and every probe loop ends");
static_assert(CW_OVL_DENSE_CAP + CW_OVL_THREADS < CW_OVL_DENSE_SLOTS, "the dense route: the same");
static_assert(CW_OVL_TABLE_WORDS(CW_OVL_SLOTS) * 4u * 3u <= 160u * 1024u - 3u * 128u && CW_OVL_TABLE_WORDS(CW_OVL_SLOTS) * 4u + 128u <= 64u * 1024u, "cw_overlap_kernel<0>: three work-groups a CU, static LDS");
static_assert(((2u * (uint32_t)CW_SW_QMAX) >> CW_SEED_SHIFT) + 1u < (1u << 11), "a bin and the bin above it fit 11 bits: reads beyond CW_SW_QMAX are no targets");
static_assert((uint64_t)CW_SW_QMAX * 128u <= (1u << 22), "a window's w is below 2^22: 22 bits of a candidate's word, and a 32-bit count never wraps");
static_assert((uint32_t)CW_SW_QMAX <= (1u << 16), "a position fits 16 bits of a posting");
static_assert(CW_STRAND_KMAX <= 15u, "a canonical k-mer is below 2^30: CW_STR_EMPTY is free, and 2^31 slots hold twice the distinct keys");

/* the table's hash: not strand_hash, whose top bits the sample has already used */
__host__ __device__ inline uint32_t ovl_hash(uint32_t key, uint32_t bits) { return ((key ^ (key >> 15)) * 0x85EBCA6Bu) >> (32u - bits); }
__device__ __forceinline__ uint32_t ovl_hash64(unsigned long long key, uint32_t bits) { return (((uint32_t)key ^ (uint32_t)(key >> 17)) * 0x9E3779B1u) >> (32u - bits); }

/* the slots of an index of n entries: a power of two, at least twice the entries or, beyond 2^30 of them, twice the keys there can be */
__host__ __device__ inline uint32_t cw_ovl_table_bits(uint64_t n) {
    uint32_t bits = 10u;
    while (bits < 31u && ((uint64_t)1 << bits) < 2u * n) ++bits;
    return bits;
}
static_assert((1u << 10) == CW_OVL_TABLE_MIN, "cw_ovl_table_bits' floor");
__host__ __device__ inline uint64_t cw_ovl_index_words(uint64_t n) { return (uint64_t)CW_OVL_HDR + 3u * ((uint64_t)1 << cw_ovl_table_bits(n)) + 2u * n; }

struct OvlIndexArgs {
    uint32_t* hdr;                 /* the index: CW_OVL_HDR words, */
    uint32_t* keys;                /* [1 << bits] */
    uint32_t* cnt;                 /* [1 << bits] */
    uint32_t* off;                 /* [1 << bits] */
    unsigned long long* post;      /* [n_entries] */
    uint64_t n_entries;            /* what the caller says cw_overlap_count_device counted */
    uint32_t bits, k, sample, max_occ, min_hits;
    uint32_t n_reads;
    const uint32_t* seq_len;       /* the read set */
    const uint64_t* seq_word_off;
    const uint32_t* bases;
    unsigned long long* counted;   /* where the count pass adds: the header's [2..3], or scratch (cw_overlap_count_device) */
};

struct OvlArgs {
    OvlIndexArgs x;
    uint32_t first, n_queries;
    int32_t* rows;                 /* the caller's */
    const uint64_t* row_off;       /* [n_queries + 1], in rows */
    uint32_t* n_rows;              /* [n_queries] */
    uint8_t* status;               /* [n_queries] */
    uint32_t* ctr;                 /* CW_OVL_CTR_WORDS scratch, zero before the run */
    uint32_t* redo;                /* [n_queries] scratch */
    uint32_t* dense;               /* [dense work-groups * CW_OVL_DENSE_WORDS] scratch */
    uint32_t* routes;              /* [2], the engine's (cw_debug_overlap_routes) */
};

/* position i of a read: 0 when it is not sampled, else 1 with *c the canonical k-mer and *s the occurrence's strand */
__device__ __forceinline__ uint32_t ovl_sampled(const uint32_t* words, uint32_t i, uint32_t k, uint32_t sample, uint32_t* c, uint32_t* s) {
    const uint32_t K = cw_kmer_at(words, i, k), R = strand_rc(K, k);
    if (K == R) return 0u;
    *c = K < R ? K : R; *s = K > R ? 1u : 0u;
    return sample == 0u || ((*c * 0x9E3779B1u) >> (32u - sample)) == 0u ? 1u : 0u;
}

__device__ __forceinline__ bool ovl_indexed(uint32_t len, uint32_t k) { return len >= k && len <= (uint32_t)CW_SW_QMAX; }

/* PASS 0 count, 1 insert, 3 fill: a work-group a read at a time, grid-stride */
template <int PASS>
__global__ void __launch_bounds__(256) cw_overlap_index_kernel(OvlIndexArgs a) {
    __shared__ uint32_t part[4];
    const uint32_t tid = threadIdx.x, k = a.k, mask = (1u << a.bits) - 1u;
    if (PASS != 0 && *(const unsigned long long*)(a.hdr + 2) != a.n_entries) return; /* the count pass ended before this launch began */
    uint32_t mine = 0;
    for (uint32_t r = blockIdx.x; r < a.n_reads; r += gridDim.x) {
        const uint32_t len = a.seq_len[r];
        if (!ovl_indexed(len, k)) continue;
        const uint32_t* const w = a.bases + a.seq_word_off[r];
        for (uint32_t i = tid; i + k <= len; i += 256u) {
            uint32_t c, s;
            if (!ovl_sampled(w, i, k, a.sample, &c, &s)) continue;
            if (PASS == 0) { ++mine; continue; }
            uint32_t h = ovl_hash(c, a.bits);
            if (PASS == 1) {
                for (;;) {
                    const uint32_t old = atomicCAS(&a.keys[h], CW_STR_EMPTY, c);
                    if (old == CW_STR_EMPTY || old == c) break;
                    h = (h + 1u) & mask;
                }
                atomicAdd(&a.cnt[h], 1u);
            } else {
                while (a.keys[h] != c) h = (h + 1u) & mask; /* it was inserted */
                const uint32_t at = atomicAdd(&a.off[h], 1u);
                if ((uint64_t)at < a.n_entries) a.post[at] = (unsigned long long)r | ((unsigned long long)i << 24) | ((unsigned long long)s << 40);
            }
        }
    }
    if (PASS == 0) {
        for (uint32_t d = 32u; d; d >>= 1) mine += __shfl_down(mine, d, 64);
        if ((tid & 63u) == 0u) part[tid >> 6] = mine;
        __syncthreads();
        if (tid == 0u) { const uint32_t sum = part[0] + part[1] + part[2] + part[3]; if (sum) atomicAdd(a.counted, (unsigned long long)sum); }
    }
}

/* a thread a slot: off[h] = where the slot's postings begin; the last pass's end marks the index as built */
__global__ void __launch_bounds__(256) cw_overlap_assign_kernel(OvlIndexArgs a) {
    __shared__ uint32_t scan[256];
    __shared__ uint32_t base;
    const uint32_t tid = threadIdx.x;
    const uint64_t slots = (uint64_t)1 << a.bits;
    if (*(const unsigned long long*)(a.hdr + 2) != a.n_entries) return;
    for (uint64_t h0 = (uint64_t)blockIdx.x * 256u; h0 < slots; h0 += (uint64_t)gridDim.x * 256u) {
        const uint32_t c = a.cnt[h0 + tid]; /* slots is a multiple of 256 */
        scan[tid] = c;
        __syncthreads();
        for (uint32_t d = 1u; d < 256u; d <<= 1) {
            const uint32_t v = tid >= d ? scan[tid - d] : 0u;
            __syncthreads();
            scan[tid] += v;
            __syncthreads();
        }
        if (tid == 255u) base = scan[255] ? atomicAdd(&a.hdr[4], scan[255]) : 0u;
        __syncthreads();
        if (c) a.off[h0 + tid] = base + scan[tid] - c;
        __syncthreads();
    }
}

__global__ void cw_overlap_seal_kernel(OvlIndexArgs a) {
    if (threadIdx.x == 0u && blockIdx.x == 0u && *(const unsigned long long*)(a.hdr + 2) == a.n_entries) a.hdr[0] = CW_OVL_MAGIC;
}

/* one vote of key into the first table; a key's first vote counts in *distinct */
__device__ __forceinline__ void ovl_count(unsigned long long* keys, uint32_t* cnt, uint32_t bits, unsigned long long key, uint32_t* distinct) {
    const uint32_t mask = (1u << bits) - 1u;
    uint32_t h = ovl_hash64(key, bits);
    for (;;) {
        const unsigned long long old = atomicCAS(&keys[h], CW_OVL_EMPTY64, key);
        if (old == CW_OVL_EMPTY64) atomicAdd(distinct, 1u);
        if (old == CW_OVL_EMPTY64 || old == key) { atomicAdd(&cnt[h], 1u); return; }
        h = (h + 1u) & mask;
    }
}

__device__ __forceinline__ uint32_t ovl_count_of(const unsigned long long* keys, const uint32_t* cnt, uint32_t bits, unsigned long long key) {
    const uint32_t mask = (1u << bits) - 1u;
    uint32_t h = ovl_hash64(key, bits);
    for (;;) {
        const unsigned long long v = keys[h];
        if (v == CW_OVL_EMPTY64) return 0u;
        if (v == key) return cnt[h];
        h = (h + 1u) & mask;
    }
}

/* the best window of (t, o) so far: the maximum of val in the second table */
__device__ __forceinline__ void ovl_best(uint32_t* k2, unsigned long long* v2, uint32_t bits, uint32_t to, unsigned long long val) {
    const uint32_t mask = (1u << bits) - 1u;
    uint32_t h = strand_hash(to, bits);
    for (;;) {
        const uint32_t old = atomicCAS(&k2[h], CW_STR_EMPTY, to);
        if (old == CW_STR_EMPTY || old == to) { atomicMax(&v2[h], val); return; }
        h = (h + 1u) & mask;
    }
}

__device__ __forceinline__ int32_t ovl_clamp(int32_t v, int32_t lo, int32_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

/* DENSE = 0: every query, the tables in LDS.  DENSE = 1: the queries of the redo list, the tables in this work-group's piece of a.dense. */
template <int DENSE>
__global__ void __launch_bounds__(CW_OVL_THREADS) cw_overlap_kernel(OvlArgs a) {
    constexpr uint32_t BITS = DENSE ? CW_OVL_DENSE_BITS : CW_OVL_BITS, SLOTS = 1u << BITS, CAP = SLOTS / 2u;
    __shared__ unsigned long long lds_tab[DENSE ? 1 : CW_OVL_TABLE_WORDS(CW_OVL_SLOTS) / 2u];
    __shared__ uint32_t claimed, distinct, n_cand;
    const uint32_t tid = threadIdx.x, k = a.x.k, mask1 = (1u << a.x.bits) - 1u;
    const uint32_t n_todo = DENSE ? a.ctr[1] : a.n_queries;
    const bool built = a.x.hdr[0] == CW_OVL_MAGIC;
    if (DENSE && blockIdx.x == 0u && tid == 0u) { a.routes[0] = a.n_queries - n_todo; a.routes[1] = n_todo; }
    unsigned long long* const keys = DENSE ? (unsigned long long*)(a.dense + (size_t)blockIdx.x * CW_OVL_DENSE_WORDS) : lds_tab;
    unsigned long long* const v2 = keys + SLOTS;
    uint32_t* const cnt = (uint32_t*)(v2 + SLOTS);
    uint32_t* const k2 = cnt + SLOTS;
    for (;;) {
        __syncthreads(); /* the query before is done with the tables and `claimed` */
        if (tid == 0) claimed = atomicAdd(&a.ctr[DENSE ? 2 : 0], 1u);
        __syncthreads();
        if (claimed >= n_todo) break;
        const uint32_t j = DENSE ? a.redo[claimed] : claimed, q = a.first + j;
        const uint32_t m = a.x.seq_len[q];
        if (!built || !ovl_indexed(m, k)) { if (tid == 0) { a.n_rows[j] = 0u; a.status[j] = (uint8_t)(built ? CW_OVL_NONE : CW_OVL_BAD_INDEX); } continue; }
        for (uint32_t x = tid; x < SLOTS; x += CW_OVL_THREADS) { keys[x] = CW_OVL_EMPTY64; v2[x] = 0ull; cnt[x] = 0u; k2[x] = CW_STR_EMPTY; }
        if (tid == 0) { distinct = 0u; n_cand = 0u; }
        if (DENSE) __threadfence(); /* the cleared words are in L2, where the other waves' atomics find them */
        __syncthreads();
        const uint32_t* const qw = a.x.bases + a.x.seq_word_off[q];
        for (uint32_t i = tid; i + k <= m; i += CW_OVL_THREADS) {
            if (*(volatile uint32_t*)&distinct > CAP) break;
            uint32_t c, sq;
            if (!ovl_sampled(qw, i, k, a.x.sample, &c, &sq)) continue;
            uint32_t h = ovl_hash(c, a.x.bits), v;
            while ((v = a.x.keys[h]) != c && v != CW_STR_EMPTY) h = (h + 1u) & mask1;
            if (v != c) continue; /* (a sampled k-mer of an indexed read is in the table; a query is an indexed read) */
            const uint32_t occ = a.x.cnt[h], end = a.x.off[h];
            if (occ > a.x.max_occ) continue;
            for (uint32_t e = end - occ; e != end; ++e) {
                if (*(volatile uint32_t*)&distinct > CAP) break; /* abandoned: at most this one more key a thread came in behind the look */
                const unsigned long long pw = a.x.post[e];
                const uint32_t t = (uint32_t)pw & 0xFFFFFFu, p = (uint32_t)(pw >> 24) & 0xFFFFu, o = sq ^ ((uint32_t)(pw >> 40) & 1u);
                if (t == q) continue;
                const uint32_t b = (o ? p + k + i : p + m - i) >> CW_SEED_SHIFT;
                ovl_count(keys, cnt, BITS, ((unsigned long long)t << 12) | (o << 11) | b, &distinct);
            }
        }
        __syncthreads();
        if (DENSE) __threadfence(); /* the atomics ran in L2: no line of the tables this CU loaded before them is read below */
        if (distinct > CAP) { /* (the count only grows: the same answer in every thread) */
            if (tid == 0) {
                if (DENSE) { a.n_rows[j] = 0u; a.status[j] = (uint8_t)CW_OVL_DENSE; }
                else a.redo[atomicAdd(&a.ctr[1], 1u)] = j;
            }
            continue;
        }
        for (uint32_t x = tid; x < SLOTS; x += CW_OVL_THREADS) {
            const unsigned long long key = keys[x];
            if (key == CW_OVL_EMPTY64) continue;
            const uint32_t b = (uint32_t)key & 0x7FFu, c = cnt[x];
            unsigned long long val = ((unsigned long long)(c + ovl_count_of(keys, cnt, BITS, key + 1u)) << 32) | (0xFFFFFFFFu - b);
            if (b >= 1u) {
                const unsigned long long down = ((unsigned long long)(ovl_count_of(keys, cnt, BITS, key - 1u) + c) << 32) | (0xFFFFFFFFu - (b - 1u));
                val = down > val ? down : val;
            }
            ovl_best(k2, v2, BITS, (uint32_t)(key >> 11), val);
        }
        __syncthreads();
        if (DENSE) __threadfence();
        unsigned long long* const list = keys; /* the first table is read no more */
        for (uint32_t x = tid; x < SLOTS; x += CW_OVL_THREADS) {
            const uint32_t to = k2[x];
            if (to == CW_STR_EMPTY) continue;
            const unsigned long long val = v2[x];
            const uint32_t w = (uint32_t)(val >> 32), b = 0xFFFFFFFFu - (uint32_t)val;
            if (w < a.x.min_hits) continue;
            list[atomicAdd(&n_cand, 1u)] = ((unsigned long long)(0x3FFFFFu - w) << 36) | ((unsigned long long)to << 11) | b;
        }
        __syncthreads();
        if (DENSE) __threadfence();
        const uint32_t nc = n_cand;
        const uint64_t r0 = a.row_off[j], cap_rows = a.row_off[j + 1] - r0;
        if (tid == 0) { a.n_rows[j] = nc; a.status[j] = (uint8_t)(nc > cap_rows ? CW_OVL_SLOT : CW_OVL_OK); }
        if (nc > cap_rows) continue;
        for (uint32_t x = tid; x < nc; x += CW_OVL_THREADS) {
            const unsigned long long me = list[x];
            uint32_t rank = 0;
            for (uint32_t y = 0; y < nc; ++y) rank += list[y] < me ? 1u : 0u;
            const uint32_t w = 0x3FFFFFu - (uint32_t)(me >> 36), t = (uint32_t)(me >> 12) & 0xFFFFFFu, o = (uint32_t)(me >> 11) & 1u, b = (uint32_t)me & 0x7FFu;
            const int32_t mm = (int32_t)m, n = (int32_t)a.x.seq_len[t], kk = (int32_t)k;
            const int32_t diag = (int32_t)(b << CW_SEED_SHIFT) - mm;
            const int32_t c0 = ovl_clamp(diag + 64, -(mm - kk), n - kk);
            const int32_t lo = c0 < 0 ? -c0 : 0, hi = mm < n - c0 ? mm : n - c0;
            int32_t* const row = a.rows + (r0 + rank) * CW_OVL_ROW;
            row[CW_OVL_TARGET] = (int32_t)t; row[CW_OVL_STRAND] = (int32_t)(o ? CW_STRAND_REV : CW_STRAND_FWD); row[CW_OVL_HITS] = (int32_t)w; row[CW_OVL_DIAG] = diag;
            row[CW_OVL_Q_START] = o ? mm - hi : lo; row[CW_OVL_Q_END] = o ? mm - 1 - lo : hi - 1;
            row[CW_OVL_T_START] = lo + c0; row[CW_OVL_T_END] = hi + c0 - 1;
        }
    }
}

/* a thread a query: its first min(n_rows, max_support, slot) rows as cw_overlap tuples; a query without rows (any status but CW_OVL_OK) gets none */
struct OvlPileArgs {
    const int32_t* rows; const uint64_t* row_off; const uint32_t* n_rows; const uint8_t* status;
    uint32_t n_queries, max_support;
    cw_overlap* pile; const uint64_t* pile_off; uint32_t* pile_n;
};
__global__ void __launch_bounds__(256) cw_overlap_to_pile_kernel(OvlPileArgs a) {
    for (uint32_t j = blockIdx.x * 256u + threadIdx.x; j < a.n_queries; j += gridDim.x * 256u) {
        const uint64_t slot = a.pile_off[j + 1] - a.pile_off[j];
        uint32_t n = a.status[j] == CW_OVL_OK ? a.n_rows[j] : 0u;
        n = n > a.max_support ? a.max_support : n;
        n = (uint64_t)n > slot ? (uint32_t)slot : n;
        a.pile_n[j] = n;
        for (uint32_t r = 0; r < n; ++r) {
            const int32_t* const row = a.rows + (a.row_off[j] + r) * CW_OVL_ROW;
            cw_overlap* const out = a.pile + a.pile_off[j] + r;
            out->q_start = (uint32_t)row[CW_OVL_Q_START]; out->q_end = (uint32_t)row[CW_OVL_Q_END]; out->t_read = (uint32_t)row[CW_OVL_TARGET];
            out->t_start = (uint32_t)row[CW_OVL_T_START]; out->t_end = (uint32_t)row[CW_OVL_T_END]; out->strand = (uint32_t)row[CW_OVL_STRAND];
        }
    }
}

#endif
