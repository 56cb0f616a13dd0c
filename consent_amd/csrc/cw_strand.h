/*
 * cw_strand.h -- both strands for the alignment operators (cw_strand_run / cw_strand_run_device, cw_revcomp / cw_revcomp_device, include/consent_amd.h): which
 * queries of a batch of groups are the reverse complement of their reference, and the batch with those queries turned round.
 *
 * The vote of a pair is a count of shared k-mers in both orientations: the reference's k-mer SET lives in LDS as an open-addressing table of 32-bit keys (a k-mer
 * of k <= CW_STRAND_KMAX = 15 bases is below 2^30, so 0xFFFFFFFF is free to mean "empty"), linear probing behind a multiplicative hash, at most half full.  A slot
 * holds the key itself and a probe compares keys, so membership is exact.  Every number is a function of the pair and k alone.
 *
 *   cw_strand_units_kernel   one work-group: the units of work of every group and their exclusive prefix sums (cw_cut_index_kernel's pattern).  A unit is (group,
 *                            chunk of its queries): a group of very many queries -- a contig with all its reads -- spreads over the GPU, the table rebuilt per
 *                            chunk.  The chunk follows the launch class: CW_STR_CHUNK = 32 queries behind a table of up to CW_ST_RMAX = 2 048 inserts (rebuild:
 *                            4 096 slots cleared and n inserts against 2 x 32 x m probes -- 6 % for a full table and 500-base queries), CW_STR_CHUNK_WIDE = 256
 *                            behind the 32 768-slot table of the wide class (rebuild: 32 768 slots and up to 16 383 inserts against 2 x 256 x m probes: 19 %).
 *                            A group of sequences has at least one unit, whose first chunk also writes the reference's own entry; a group of none has none.
 *   cw_strand_kernel<WIDE>   a fixed grid that claims units from a counter in scratch.  WIDE = 0: references of up to CW_ST_RMAX bases, a 4 096-slot table in 16 KB
 *                            of static LDS, 256 threads, several work-groups a CU; WIDE = 1: references of up to CW_SW_RMAX, a 32 768-slot table in 128 KB of
 *                            dynamic LDS, 1 024 threads, one work-group a CU.  Each launch skips the other class's groups (the host does not know the lengths of a
 *                            device batch), and ends at once when the units kernel counted none of its class.  Per unit: the table is cleared, the threads insert
 *                            the reference's k-mers with LDS compare-and-swap, then the waves take the chunk's queries in turn, the lanes over positions: a lane
 *                            cuts the k-mer at position i from two neighbouring packed words with one 64-bit shift (cw_kmer_at), probes it, probes its reverse
 *                            complement (bit-reverse, swap of neighbouring bits, complement, shift), the wave sums the two counts and lane 0 stores the entry.
 *   cw_revcomp_kernel        sixteen lanes a sequence, over its output words: output word w of a reversed sequence is the 32-bit window of the input that ends at
 *                            base len - 1 - 16 w -- a funnel shift over at most two input words -- bit-reversed, neighbouring bits swapped, complemented, and the
 *                            last word masked to its bases.  An unflagged sequence's words are copied.  Memory-bound by construction: a word read, a word written.
 *                            (Handing the words a sequence has beyond its first 64 to the whole work-group was measured and was slower on every shape.)
 *
 * No inline assembly, plain C++ stores only, no environment switch.
 */
#ifndef CW_STRAND_H
#define CW_STRAND_H

#include "cw_device.h"
#include "cw_stitch.h" /* CW_ST_RMAX: the reference length at which the aligner, too, changes class */

#define CW_STR_EMPTY 0xFFFFFFFFu
#define CW_STR_SLOTS 4096u        /* 16 KB: references of up to CW_ST_RMAX bases */
#define CW_STR_SLOTS_WIDE 32768u  /* 128 KB: references of up to CW_SW_RMAX */
#define CW_STR_CHUNK 32u          /* queries a unit */
#define CW_STR_CHUNK_WIDE 256u
#define CW_STR_THREADS 256
#define CW_STR_THREADS_WIDE 1024
#define CW_STR_CTR_WORDS 8u       /* [0], [1]: the claim counters of the two launches; [2], [3]: the units of each class */
#define CW_RC_LANES 16u           /* lanes a sequence of the reverse-complement kernel */

static_assert(2u * CW_ST_RMAX <= CW_STR_SLOTS && 2u * CW_SW_RMAX <= CW_STR_SLOTS_WIDE, "a table is at most half full");
static_assert(CW_STRAND_KMAX <= 15u && CW_STRAND_KMIN >= 1u && CW_STRAND_K >= CW_STRAND_KMIN && CW_STRAND_K <= CW_STRAND_KMAX, "a k-mer is below 2^30: one 32-bit key with a free empty value");
static_assert(CW_STR_SLOTS_WIDE * 4u <= 160u * 1024u - 1024u, "the wide table and the claimed unit in a work-group's LDS");

struct StrandArgs {
    DevBatch b;
    uint32_t n_seqs;
    uint8_t* strand;    /* [n_seqs], the caller's */
    uint32_t* hits;     /* [n_seqs * 2] or NULL */
    uint32_t k;         /* CW_STRAND_KMIN .. CW_STRAND_KMAX */
    uint32_t* unit_off; /* [n_windows + 1] scratch: the first unit of every group; [n_windows] = units */
    uint32_t* ctr;      /* CW_STR_CTR_WORDS scratch, zero before the run */
};

/* the launch class of a group by its reference's length, and the queries of one of its units */
__device__ __forceinline__ uint32_t strand_class(uint32_t n) { return n > (uint32_t)CW_ST_RMAX ? 1u : 0u; }
__device__ __forceinline__ uint32_t strand_chunk(uint32_t n) { return strand_class(n) ? CW_STR_CHUNK_WIDE : CW_STR_CHUNK; }

/* one work-group: units per group and their exclusive prefix sums, and the units of each class */
__global__ void __launch_bounds__(1024) cw_strand_units_kernel(StrandArgs a) {
    __shared__ uint32_t ps[1024];
    __shared__ uint32_t run, per_class[2];
    const int tid = threadIdx.x;
    if (tid == 0) { run = 0; per_class[0] = 0; per_class[1] = 0; }
    __syncthreads();
    for (uint32_t g0 = 0; g0 < a.b.n_windows; g0 += 1024) {
        const uint32_t g = g0 + tid;
        uint32_t u = 0;
        if (g < a.b.n_windows) {
            const uint32_t r = a.b.win_first_seq[g], q_end = a.b.win_first_seq[g + 1];
            if (r < q_end) {
                const uint32_t n = a.b.seq_len[r], chunk = strand_chunk(n), nq = q_end - r - 1u;
                u = nq ? (nq + chunk - 1u) / chunk : 1u;
                atomicAdd(&per_class[strand_class(n)], u);
            }
        }
        ps[tid] = u;
        __syncthreads();
        for (int o = 1; o < 1024; o <<= 1) {
            uint32_t v = 0;
            if (tid >= o) v = ps[tid - o];
            __syncthreads();
            ps[tid] += v;
            __syncthreads();
        }
        if (g < a.b.n_windows) a.unit_off[g] = run + ps[tid] - u;
        __syncthreads();
        if (tid == 0) run += ps[1023];
        __syncthreads();
    }
    if (tid == 0) { a.unit_off[a.b.n_windows] = run; a.ctr[2] = per_class[0]; a.ctr[3] = per_class[1]; }
}

__device__ __forceinline__ uint32_t strand_hash(uint32_t key, uint32_t bits) { return (key * 0x9E3779B1u) >> (32u - bits); }

/* the reverse complement of a k-mer: bit-reverse (the bases in reverse order, the two bits of each swapped), swap them back, complement, down to 2k bits */
__device__ __forceinline__ uint32_t strand_rc(uint32_t x, uint32_t k) {
    const uint32_t r = __brev(x);
    return ~(((r & 0x55555555u) << 1) | ((r >> 1) & 0x55555555u)) >> (32u - 2u * k);
}

/* whether key is in the table: the slots from its hash on hold it, or another key, until an empty one -- there is one, the table being at most half full */
template <uint32_t SLOTS, uint32_t BITS>
__device__ __forceinline__ uint32_t strand_has(const uint32_t* tab, uint32_t key) {
    uint32_t h = strand_hash(key, BITS);
    for (;;) {
        const uint32_t v = tab[h];
        if (v == key) return 1u;
        if (v == CW_STR_EMPTY) return 0u;
        h = (h + 1u) & (SLOTS - 1u);
    }
}

__device__ __forceinline__ void strand_store(const StrandArgs& a, uint32_t s, uint32_t strand, uint32_t fwd, uint32_t rev) {
    a.strand[s] = (uint8_t)strand;
    if (a.hits) { a.hits[2u * (size_t)s] = fwd; a.hits[2u * (size_t)s + 1u] = rev; }
}

template <int WIDE>
__global__ void __launch_bounds__(WIDE ? CW_STR_THREADS_WIDE : CW_STR_THREADS) cw_strand_kernel(StrandArgs a) {
    constexpr uint32_t SLOTS = WIDE ? CW_STR_SLOTS_WIDE : CW_STR_SLOTS, BITS = WIDE ? 15u : 12u, THREADS = WIDE ? CW_STR_THREADS_WIDE : CW_STR_THREADS;
    static_assert((1u << BITS) == SLOTS, "the hash gives a slot");
    extern __shared__ uint32_t strand_dyn[];
    __shared__ uint32_t tab_static[WIDE ? 1 : CW_STR_SLOTS];
    __shared__ uint32_t claimed;
    uint32_t* const tab = WIDE ? strand_dyn : tab_static;
    if (a.ctr[2 + WIDE] == 0u) return; /* no group of this class */
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, k = a.k;
    const uint32_t n_units = a.unit_off[a.b.n_windows];
    for (;;) {
        __syncthreads(); /* the unit before is done with the table and with `claimed` */
        if (tid == 0) claimed = atomicAdd(&a.ctr[WIDE], 1u);
        __syncthreads();
        const uint32_t u = claimed;
        if (u >= n_units) break;
        uint32_t lo = 0, hi = a.b.n_windows; /* the group of u: the last with unit_off[g] <= u (a group of none shares its successor's offset) */
        while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (a.unit_off[mid] <= u) lo = mid; else hi = mid; }
        const uint32_t r = a.b.win_first_seq[lo], q_end = a.b.win_first_seq[lo + 1];
        const uint32_t n = a.b.seq_len[r];
        if (strand_class(n) != (uint32_t)WIDE) continue; /* the other launch's */
        const uint32_t c = u - a.unit_off[lo], chunk = strand_chunk(n);
        const uint32_t s0 = r + 1u + c * chunk, s1 = q_end - s0 > chunk ? s0 + chunk : q_end; /* (s0 <= q_end: c is below the group's units) */
        if (c == 0u && tid == 0u) strand_store(a, r, CW_STRAND_IS_REF, 0u, 0u);
        if (n < k || n > (uint32_t)CW_SW_RMAX) { /* no vote against this reference */
            for (uint32_t s = s0 + tid; s < s1; s += THREADS) strand_store(a, s, CW_STRAND_NONE, 0u, 0u);
            continue;
        }
        for (uint32_t x = tid; x < SLOTS; x += THREADS) tab[x] = CW_STR_EMPTY;
        __syncthreads();
        const uint32_t* const rw = a.b.bases + a.b.seq_word_off[r];
        for (uint32_t j = tid; j + k <= n; j += THREADS) {
            const uint32_t key = cw_kmer_at(rw, j, k);
            uint32_t h = strand_hash(key, BITS);
            for (;;) {
                const uint32_t old = atomicCAS(&tab[h], CW_STR_EMPTY, key);
                if (old == CW_STR_EMPTY || old == key) break;
                h = (h + 1u) & (SLOTS - 1u);
            }
        }
        __syncthreads();
        for (uint32_t s = s0 + wave; s < s1; s += THREADS / 64u) { /* a query a wave, the lanes over its positions */
            const uint32_t m = a.b.seq_len[s];
            if (m < k || m > (uint32_t)CW_SW_QMAX) { if (lane == 0u) strand_store(a, s, CW_STRAND_NONE, 0u, 0u); continue; }
            const uint32_t* const qw = a.b.bases + a.b.seq_word_off[s];
            uint32_t fwd = 0, rev = 0;
            for (uint32_t i = lane; i + k <= m; i += 64u) {
                const uint32_t key = cw_kmer_at(qw, i, k);
                fwd += strand_has<SLOTS, BITS>(tab, key);
                rev += strand_has<SLOTS, BITS>(tab, strand_rc(key, k));
            }
            const uint32_t f = (uint32_t)cw_wave_sum((int)fwd), v = (uint32_t)cw_wave_sum((int)rev);
            if (lane == 0u) strand_store(a, s, v > f ? CW_STRAND_REV : CW_STRAND_FWD, f, v);
        }
    }
}

/* ---- cw_revcomp: the oriented batch's words ------------------------------------------------------------------------------------------------------------------- */

struct RevcompArgs {
    uint32_t n_seqs;
    const uint32_t* seq_len;
    const uint64_t* seq_word_off;
    const uint32_t* bases;
    const uint8_t* strand; /* NULL: every sequence is reversed */
    uint32_t* out;
};

/* output word w of the reverse complement of len bases in `in`: the 16 bases that end at base hi = len - 1 - 16 w */
__device__ __forceinline__ uint32_t revcomp_word(const uint32_t* in, uint32_t len, uint32_t w) {
    const uint32_t hi = len - 1u - 16u * w, wi = hi >> 4, r = (hi & 15u) + 1u; /* r bases of word wi, 16 - r of the word before it */
    const uint32_t a = wi ? in[wi - 1u] : 0u, b = in[wi];
    const uint32_t x = (uint32_t)((((uint64_t)a << 32) | b) >> (32u - 2u * r)); /* the funnel shift: base hi in the lowest two bits */
    const uint32_t v = __brev(x);
    const uint32_t y = ~(((v & 0x55555555u) << 1) | ((v >> 1) & 0x55555555u));
    const uint32_t nb = len - 16u * w; /* the bases of this word: fewer than 16 in the last one only */
    return nb < 16u ? y & ~(0xFFFFFFFFu >> (2u * nb)) : y;
}

__global__ void __launch_bounds__(256) cw_revcomp_kernel(RevcompArgs a) {
    const uint32_t sub = threadIdx.x % CW_RC_LANES, per = 256u / CW_RC_LANES;
    for (uint64_t s = (uint64_t)blockIdx.x * per + threadIdx.x / CW_RC_LANES; s < a.n_seqs; s += (uint64_t)gridDim.x * per) {
        const uint32_t len = a.seq_len[s], nw = (len + 15u) / 16u;
        const uint32_t* const in = a.bases + a.seq_word_off[s];
        uint32_t* const out = a.out + a.seq_word_off[s];
        const bool turn = !a.strand || a.strand[s] == CW_STRAND_REV;
        for (uint32_t w = sub; w < nw; w += CW_RC_LANES) out[w] = turn ? revcomp_word(in, len, w) : in[w];
    }
}

#endif
