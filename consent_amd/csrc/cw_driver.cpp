/*
 * cw_driver.cpp -- the loop of CONSENT's two drivers behind one C entry point, cw_run_correction:
 *
 *   runCorrection / processRead    (src/CONSENT-correction.cpp:62-135, :19-58)   polishing = 0
 *   runCorrection / processContig  (src/CONSENT-polishing.cpp:107-135, :21-105)  polishing = 1 (never trims, :19)
 *
 * Same inputs (the flags of src/main.cpp:29-76), same output: FASTA records ">name\nsequence\n" in PAF order, nothing for a read
 * without windows or dropped by the 10 % rule (CONSENT-correction.cpp:23-25, :52-56, :101-103).
 *
 * Shape: ONE host process; the calling thread reads the PAF pile by pile (cw_paf_next_pile), cuts the windows
 * (cw_window_positions) and packs piles into jobs of ~32k windows; one worker thread per device owns an engine and a copy of the
 * 2-bit read set and pulls jobs from a bounded queue (dynamic: a device that finishes early takes the next job); per job the piles
 * never leave the device: cw_extract_piles_device -> cw_plan_results_device -> cw_run_device -> cw_stitch_device, and only the
 * corrected reads come back.  An emitter thread writes finished jobs in submission order, so the output does not depend on the
 * number of devices.  No collective: jobs are independent.
 *
 * Host code only (device memory through the HIP runtime API); everything that computes is behind the C ABI of consent_amd.h.
 */
#include "cw_internal.h"
#include "cw_private.h"
#include "cw_device.h"      /* CwProfSlot, BatchCounters: what cw_debug_profile's words are (print_job_profile) */
#include "cw_driver_plan.h"

#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <future>
#include <map>
#include <string>
#include <thread>
#include <vector>

namespace {

struct Job {
    uint64_t seq = 0;
    std::vector<cw_overlap> ovl;
    std::vector<cw_window_job> wj;
    std::vector<uint32_t> win_pos;   /* (beg, end) per window */
    std::vector<cw_stitch_read> sr;  /* one per pile */
    uint64_t cost = 0;               /* sum over windows of (overlaps + 1): what the shard balance goes by */
    /* results */
    std::vector<std::string> out;    /* per pile; "" = no record */
    int rc = CW_OK;
    std::string err;
    int device = -1;
    double ms_extract = 0, ms_consensus = 0, ms_stitch = 0;
};

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes) {
        if (bytes <= cap) return CW_OK;
        if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
        const size_t want = bytes + bytes / 2 + 256; /* half again: a regrowth is a hipFree + hipMalloc, both of which wait for the device (and for the other worker's kernels on it) */
        if (hipMalloc(&p, want) != hipSuccess) { p = nullptr; return CW_E_NOMEM; }
        cap = want;
        return CW_OK;
    }
    ~DevBuf() { if (p) (void)hipFree(p); }
    template <typename T> T* as() const { return (T*)p; }
};

struct Shared {
    const cw_driver_args* a = nullptr;
    cw_read_index* index = nullptr;
    cw_read_set host_reads{};
    uint64_t read_words = 0;
    double t_start = 0; /* now_ms() when the run began (statistics, inspection output) */
    bool do_trim = true;
    bool skip_on_capacity = false;
    bool dry = false; /* CW_DRIVER_DRY: workers take the jobs and throw them away -- what the host side alone can feed (no device is touched) */
    /* job queue (producer -> workers) */
    std::mutex mu;
    std::condition_variable cv_work, cv_room, cv_done;
    std::deque<Job*> queue;
    size_t queue_cap = 4;
    bool closed = false; /* the producer is done: n_jobs_total is final */
    uint64_t n_jobs_total = 0;
    /* finished jobs, keyed by sequence number (workers -> emitter) */
    std::map<uint64_t, Job*> finished;
    std::atomic<bool> abort{false}; /* written under mu, also read outside it by the producer loop */
    int first_error = CW_OK;
    std::string first_error_msg;
    /* the first error is the run's; whoever waits -- workers, producer, emitter -- wakes and sees abort.  Called with mu held. */
    void fail(int rc, const std::string& msg) {
        if (first_error == CW_OK) { first_error = rc; first_error_msg = msg; }
        abort = true;
        cv_work.notify_all(); cv_room.notify_all(); cv_done.notify_all();
    }
};

double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

/* what a phase of Worker::process returns: CW_OK, or the job's status with the step that failed */
int job_hip(hipError_t e, Job& j, const char* what) { if (e != hipSuccess) { j.rc = CW_E_NO_DEVICE; j.err = what; } return e != hipSuccess; }
int job_rc(int rc, Job& j, const char* what) { if (rc != CW_OK) { j.rc = rc; j.err = what; } return rc != CW_OK; }

/* words of cw_debug_profile's counters (BatchCounters, cw_device.h): tasks, members, then per POA tier the tasks routed to it and the tasks that outgrew into it */
enum : uint32_t { CTR_TASKS = offsetof(BatchCounters, n_tasks) / 4, CTR_MEMBERS = offsetof(BatchCounters, n_members) / 4, CTR_N_TIER = offsetof(BatchCounters, n_tier) / 4,
                  CTR_N_OVER = offsetof(BatchCounters, n_over) / 4, CTR_WORDS = offsetof(BatchCounters, done_wgs) / 4 };
static_assert(CTR_TASKS == 0 && CTR_MEMBERS == 1 && CTR_N_TIER == 6 && CTR_N_OVER == 18 && CTR_WORDS == 30, "cw_debug_profile's counter words (cw_private.h)");
enum { TIER_Q = 0, TIER_S = 0, TIER_M1 = 1, TIER_M2 = 2, TIER_L = 3, TIER_G = 4 }; /* (list 0 is tier Q's when tasks are routed, tier S's when they outgrow: cw_device.h CW_TIERS) */

/* CW_DRIVER_PROFILE: how the job's POA tasks spread over the tiers, and where tier L's time went; with CW_TASK_TRACE the timeline of the slab tiers (inspection) */
void print_job_profile(cw_engine* eng, uint64_t job_seq, uint32_t n_win) {
    const unsigned long long seq = job_seq;
    uint32_t c[CTR_WORDS] = {0}; unsigned long long pr[72] = {0};
    const int L = CW_PS_POA + CW_PS_POA_STRIDE * TIER_L; /* tier L's phases: metadata, fill, traceback, merge */
    if (cw_debug_profile(eng, c, CTR_WORDS, pr, 72, nullptr, nullptr) == CW_OK)
        fprintf(stderr, "[job %llu] windows %u tasks %u members %u | routed Q %u M1 %u M2 %u L %u, outgrew into S %u L %u G %u | L Mcycles meta %.0f fill %.0f trace %.0f merge %.0f, rows %llu chunk-rows %llu, longest task M1 %.1f M2 %.1f L %.1f Mcycles\n",
                seq, n_win, c[CTR_TASKS], c[CTR_MEMBERS], c[CTR_N_TIER + TIER_Q], c[CTR_N_TIER + TIER_M1], c[CTR_N_TIER + TIER_M2], c[CTR_N_TIER + TIER_L], c[CTR_N_OVER + TIER_S], c[CTR_N_OVER + TIER_L],
                c[CTR_N_OVER + TIER_G], pr[L] / 1e6, pr[L + 1] / 1e6, pr[L + 2] / 1e6, pr[L + 3] / 1e6, pr[CW_PS_L_ROWS], pr[CW_PS_L_CHUNK_ROWS], pr[CW_PS_LONGEST + TIER_M1] / 1e6,
                pr[CW_PS_LONGEST + TIER_M2] / 1e6, pr[CW_PS_LONGEST + TIER_L] / 1e6);
    if (!getenv("CW_TASK_TRACE")) return; /* timeline of the slab tiers: when their tasks ran (10 ns units since the tier sort) */
    std::vector<uint32_t> tr((size_t)c[CTR_TASKS] * 12 + 12);
    uint32_t nt = 0;
    if (cw_debug_task_trace(eng, c[CTR_TASKS], tr.data(), &nt) != CW_OK) return;
    for (uint32_t tier = 1; tier <= 3; ++tier) {
        double busy = 0, first = 1e30, last = 0, longest = 0; uint32_t cnt = 0;
        for (uint32_t i = 0; i < nt; ++i) {
            const uint32_t* q = &tr[(size_t)i * 12];
            if ((q[10] & 0xFF) != tier || q[9] == 0) continue;
            const double st_ = q[8] * 1e-5, du = q[9] * 1e-5;
            busy += du; first = st_ < first ? st_ : first; last = st_ + du > last ? st_ + du : last; longest = du > longest ? du : longest; ++cnt;
        }
        if (!cnt) continue;
        int occ[9] = {0};
        for (uint32_t i = 0; i < nt; ++i) {
            const uint32_t* q = &tr[(size_t)i * 12];
            if ((q[10] & 0xFF) != tier || q[9] == 0) continue;
            const double st_ = q[8] * 1e-5, en = st_ + q[9] * 1e-5;
            for (int k = 1; k <= 9; ++k) { const double at = last * k / 10.0; if (st_ < at && en > at) occ[k - 1]++; }
        }
        if (tier == 3) { /* the three runs that ended last */
            for (int rep = 0; rep < 3; ++rep) {
                double best = -1; uint32_t bi = 0;
                for (uint32_t i = 0; i < nt; ++i) {
                    const uint32_t* q = &tr[(size_t)i * 12];
                    if ((q[10] & 0xFF) != tier || q[9] == 0) continue;
                    const double en = (q[8] + (double)q[9]) * 1e-5;
                    if (en > best && en < last + 1 - rep * 1e-9 && (rep == 0 || en < last)) { best = en; bi = i; }
                }
                const uint32_t* q = &tr[(size_t)bi * 12];
                fprintf(stderr, "[job %llu]    ends %.2f start %.2f dur %.2f ms members %u max_len %u mean_len %u rc %u pass %u wave %u\n", seq, best,
                        q[8] * 1e-5, q[9] * 1e-5, q[3], q[4] & 0xFFFF, q[4] >> 16, (q[10] >> 8) & 0xFF, q[10] >> 16, q[11]);
                last = best;
            }
        }
        fprintf(stderr, "[job %llu] tier %u: %u runs, busy %.0f wave-ms, first start %.2f, last end %.2f ms, longest %.2f ms; running at 10..90 %% of its span: %d %d %d %d %d %d %d %d %d\n",
                seq, tier, cnt, busy, first, last, longest, occ[0], occ[1], occ[2], occ[3], occ[4], occ[5], occ[6], occ[7], occ[8]);
    }
}

/* What the phases of one job share (Worker::process).  Copies queued on the worker's stream read and write these vectors and those of the Job. */
struct JobState {
    struct Slice { uint32_t w0, w1, n_seqs; uint64_t n_words, seq_base, word_base; };
    uint32_t n_win = 0, n_piles = 0, run_windows = 0;
    std::vector<Slice> slices;
    cw_batch batch{};
    cw_result res{};
    std::vector<uint64_t> out_off;   /* every read's slot in the output buffer */
    std::vector<uint32_t> h_len;     /* host-side landing: corrected length and status per read, status per window */
    std::vector<uint8_t> h_st, h_wst;
    std::vector<char> tainted;       /* reads left out, or the run's error: a capacity of the engine was exceeded */
    double t_alloc = 0, t_stitch = 0; /* result planning + allocation (inspection); when the re-assembly began */
};

struct Worker {
    int device = 0; /* the device this worker serves: read-set ownership, statistics */
    int phys = 0;   /* the HIP device behind it (== device, except under the test aid CW_VIRTUAL_DEVICES: several logical devices on one GPU) */
    cw_engine* eng = nullptr;
    hipStream_t st = nullptr;
    cw_read_set dev_reads{};
    DevBuf rd_len, rd_off, rd_bases;
    void* pin = nullptr; /* pinned landing buffer for the corrected reads */
    size_t pin_cap = 0;
    struct { DevBuf ovl, wj, pos, sr; } in;                                   /* the job as the producer cut it: overlaps, window jobs, window positions, reads */
    struct { DevBuf wfs, len, off, bases; } b;                                /* the batch: the piles of every window, cut on the device */
    struct { DevBuf cons, coff, clen, stat, solid, soff, slen; } r;           /* results per window */
    struct { DevBuf buf, off, len, stat; } o;                                 /* output: the corrected reads */
    uint64_t windows = 0, reads = 0, jobs = 0;
    double ms_extract = 0, ms_consensus = 0, ms_stitch = 0;

    /* The 2-bit read set is uploaded once per DEVICE: the first worker on a device owns the copy and publishes it, the others on that
       device (two workers per GPU by default) wait for it and use the same buffers. */
    std::promise<int> reads_ready;            /* set by an owner, in every path out of init() */
    std::shared_future<int> reads_of_owner;   /* valid in a worker that borrows another worker's copy */
    const Worker* owner = nullptr;

    int upload_reads(const Shared& sh) {
        const uint32_t n = sh.host_reads.n_reads;
        int rc;
        if ((rc = rd_len.ensure((size_t)n * 4 + 4)) || (rc = rd_off.ensure((size_t)n * 8 + 8)) || (rc = rd_bases.ensure((size_t)sh.read_words * 4 + 8))) return rc;
        if (hipMemcpy(rd_len.p, sh.host_reads.read_len, (size_t)n * 4, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(rd_off.p, sh.host_reads.read_word_off, (size_t)n * 8, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(rd_bases.p, sh.host_reads.bases, (size_t)sh.read_words * 4, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemset((uint8_t*)rd_bases.p + (size_t)sh.read_words * 4, 0, 8) != hipSuccess)
            return CW_E_NO_DEVICE;
        dev_reads.n_reads = n;
        dev_reads.read_len = rd_len.as<uint32_t>();
        dev_reads.read_word_off = rd_off.as<uint64_t>();
        dev_reads.bases = rd_bases.as<uint32_t>();
        return CW_OK;
    }

    int init(const Shared& sh) {
        int rc = CW_OK;
        if (sh.dry) { if (!owner) reads_ready.set_value(CW_OK); return CW_OK; }
        if (hipSetDevice(phys) != hipSuccess) rc = CW_E_NO_DEVICE;
        if (!owner) { /* the copy first: the borrowers' engines are being created meanwhile */
            if (rc == CW_OK) rc = upload_reads(sh);
            reads_ready.set_value(rc);
        }
        if (rc != CW_OK) return rc;
        const cw_driver_args& a = *sh.a;
        cw_params prm{a.mer_size, a.solid_thresh, a.common_kmers, a.min_anchors, a.max_msa};
        rc = cw_create(&prm, phys, &eng);
        if (rc != CW_OK) return rc;
        /* templates are windows: at most window_size bases -- longer than the default plan assumes, or shorter (beyond what the engine takes at all, every
           window reports its capacity as before: CW_WHY_TEMPLATE) */
        (void)cw_configure(eng, a.window_size);
        if (hipStreamCreate(&st) != hipSuccess) return CW_E_NO_DEVICE;
        if (owner) {
            if ((rc = reads_of_owner.get()) != CW_OK) return rc;
            dev_reads = owner->dev_reads;
        }
        return CW_OK;
    }

    void close() {
        if (!eng && !st && !pin) return; /* nothing was created (dry run, or init failed early) */
        (void)hipSetDevice(phys);
        if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); st = nullptr; }
        if (pin) { (void)hipHostFree(pin); pin = nullptr; pin_cap = 0; }
        if (eng) { cw_destroy(eng); eng = nullptr; }
    }


    int upload_job(Job& j, JobState& s) {
        const uint32_t n_win = s.n_win, n_piles = s.n_piles;
        if (job_hip(hipSetDevice(phys), j, "hipSetDevice")) return j.rc;
        if (job_rc(in.ovl.ensure(j.ovl.size() * sizeof(cw_overlap) + 64), j, "device memory (overlaps)") || job_rc(in.wj.ensure((size_t)n_win * sizeof(cw_window_job)), j, "device memory (window jobs)") ||
            job_rc(in.pos.ensure((size_t)n_win * 8), j, "device memory (window positions)") || job_rc(in.sr.ensure((size_t)n_piles * sizeof(cw_stitch_read)), j, "device memory (reads)"))
            return j.rc;
        if (!j.ovl.empty() && job_hip(hipMemcpyAsync(in.ovl.p, j.ovl.data(), j.ovl.size() * sizeof(cw_overlap), hipMemcpyHostToDevice, st), j, "H2D overlaps")) return j.rc;
        if (job_hip(hipMemcpyAsync(in.wj.p, j.wj.data(), (size_t)n_win * sizeof(cw_window_job), hipMemcpyHostToDevice, st), j, "H2D jobs") ||
            job_hip(hipMemcpyAsync(in.pos.p, j.win_pos.data(), (size_t)n_win * 8, hipMemcpyHostToDevice, st), j, "H2D positions") ||
            job_hip(hipMemcpyAsync(in.sr.p, j.sr.data(), (size_t)n_piles * sizeof(cw_stitch_read), hipMemcpyHostToDevice, st), j, "H2D reads"))
            return j.rc;
        return CW_OK;
    }

    /* ---- piles, cut on the device ----
       A job's windows are extracted in slices (the extraction keeps one descriptor per window and overlap of its pile: a slice stays
       under 2^26 of them) into ONE batch in device memory -- every slice writes window -> sequence and sequence -> word offsets that
       start at zero, which cw_add_offsets_device then moves to the slice's place -- and corrected in runs of at most CW_MAX_BATCH_WINDOWS
       windows over that batch (a run names its windows by pointer; sequence indices and word offsets are the batch's), results into
       one set of arrays planned for the whole job.  The re-assembly then walks each read's windows over the whole job, so a read --
       or a contig of any length -- may span slices and runs.  (Usually: one slice, one run.) */
    int extract(const Shared& sh, Job& j, JobState& s) {
        const cw_driver_args& a = *sh.a;
        const uint32_t n_win = s.n_win;
        uint64_t desc_budget = 1ull << 26;
        uint32_t run_windows = cw_max_batch_windows(eng); /* (CW_MAX_BATCH_WINDOWS, fewer for long windows: include/consent_amd.h) */
        if (const char* env = CW_AID_ENV("CW_DRIVER_SLICE_DESC")) { const long long v = atoll(env); if (v >= 1) desc_budget = (uint64_t)v; }           /* test aids */
        if (const char* env = CW_AID_ENV("CW_DRIVER_RUN_WINDOWS")) { const long v = atol(env); if (v >= 1 && v < (long)run_windows) run_windows = (uint32_t)v; }
        s.run_windows = run_windows;
        uint64_t tot_seqs = 0, tot_words = 0;
        for (uint32_t w0 = 0; w0 < n_win;) {
            uint64_t d = 0;
            uint32_t w1 = w0;
            while (w1 < n_win && w1 - w0 < run_windows && (w1 == w0 || d + j.wj[w1].ovl_count + 1 <= desc_budget)) { d += j.wj[w1].ovl_count + 1; ++w1; }
            JobState::Slice sl{w0, w1, 0, 0, tot_seqs, tot_words};
            const int rc = cw_extract_impl(eng, &dev_reads, in.ovl.as<cw_overlap>(), j.ovl.size(), in.wj.as<cw_window_job>() + w0, j.wj.data() + w0, w1 - w0, a.mer_size, nullptr, nullptr,
                                           nullptr, nullptr, 0, 0, &sl.n_seqs, &sl.n_words, st);
            if (rc != CW_OK && rc != CW_E_CAPACITY) { j.rc = rc; j.err = "cw_extract_piles_device (sizing)"; return rc; }
            tot_seqs += sl.n_seqs; tot_words += sl.n_words;
            s.slices.push_back(sl);
            w0 = w1;
        }
        if (tot_seqs > 0xFFFFFFF0ull) { j.rc = CW_E_CAPACITY; j.err = "more than 2^32 pile sequences in one job"; return j.rc; }
        if (job_rc(b.wfs.ensure((size_t)(n_win + 1) * 4), j, "device memory (batch)") || job_rc(b.len.ensure((size_t)tot_seqs * 4 + 4), j, "device memory (batch)") ||
            job_rc(b.off.ensure((size_t)tot_seqs * 8 + 8), j, "device memory (batch)") || job_rc(b.bases.ensure((size_t)tot_words * 4 + 8), j, "device memory (batch)") ||
            job_hip(hipMemsetAsync((uint8_t*)b.bases.p + (size_t)tot_words * 4, 0, 8, st), j, "memset"))
            return j.rc;
        for (const JobState::Slice& sl : s.slices) {
            uint32_t ns = 0; uint64_t nw = 0;
            if (job_rc(cw_extract_impl(eng, &dev_reads, in.ovl.as<cw_overlap>(), j.ovl.size(), in.wj.as<cw_window_job>() + sl.w0, j.wj.data() + sl.w0, sl.w1 - sl.w0, a.mer_size,
                                       b.wfs.as<uint32_t>() + sl.w0, b.len.as<uint32_t>() + sl.seq_base, b.off.as<uint64_t>() + sl.seq_base, b.bases.as<uint32_t>() + sl.word_base,
                                       sl.n_seqs, sl.n_words, &ns, &nw, st),
                       j, "cw_extract_piles_device") ||
                job_rc(cw_add_offsets_device(b.wfs.as<uint32_t>() + sl.w0, (uint64_t)(sl.w1 - sl.w0) + 1, (uint32_t)sl.seq_base, b.off.as<uint64_t>() + sl.seq_base, sl.n_seqs, sl.word_base, st),
                       j, "cw_add_offsets_device"))
                return j.rc;
        }
        s.batch = cw_batch{n_win, (uint32_t)tot_seqs, tot_words, b.wfs.as<uint32_t>(), b.len.as<uint32_t>(), b.off.as<uint64_t>(), b.bases.as<uint32_t>()};
        return CW_OK;
    }

    /* ---- consensus per window ---- */
    int consensus(Job& j, JobState& s) {
        const uint32_t n_win = s.n_win, run_windows = s.run_windows;
        const std::vector<JobState::Slice>& slices = s.slices;
        const double t_a0 = now_ms();
        if (job_rc(r.coff.ensure((size_t)(n_win + 1) * 8), j, "device memory (results)") || job_rc(r.soff.ensure((size_t)(n_win + 1) * 8), j, "device memory (results)")) return j.rc;
        uint64_t cons_total = 0, solid_total = 0;
        if (job_rc(cw_plan_results_device(eng, &s.batch, r.coff.as<uint64_t>(), r.soff.as<uint64_t>(), &cons_total, &solid_total, st), j, "cw_plan_results_device")) return j.rc;
        if (job_rc(r.cons.ensure(cons_total + 16), j, "device memory (results)") || job_rc(r.solid.ensure(solid_total * 4 + 16), j, "device memory (results)") ||
            job_rc(r.clen.ensure((size_t)n_win * 4), j, "device memory (results)") || job_rc(r.slen.ensure((size_t)n_win * 4), j, "device memory (results)") ||
            job_rc(r.stat.ensure(n_win), j, "device memory (results)") || job_hip(hipMemsetAsync(r.stat.p, 0xFF, n_win, st), j, "memset"))
            return j.rc;
        s.res = cw_result{r.cons.as<char>(), r.coff.as<uint64_t>(), r.clen.as<uint32_t>(), r.stat.as<uint8_t>(), r.solid.as<uint32_t>(), r.soff.as<uint64_t>(), r.slen.as<uint32_t>()};
        s.t_alloc = now_ms() - t_a0; /* result planning + allocation (inspection) */
        for (size_t s0 = 0; s0 < slices.size();) { /* runs = whole slices, at most run_windows windows */
            size_t s1 = s0 + 1;
            while (s1 < slices.size() && slices[s1].w1 - slices[s0].w0 <= run_windows) ++s1;
            const uint32_t w0 = slices[s0].w0, w1 = slices[s1 - 1].w1;
            uint64_t rs = 0, rw = 0;
            for (size_t x = s0; x < s1; ++x) { rs += slices[x].n_seqs; rw += slices[x].n_words; }
            cw_batch run{w1 - w0, (uint32_t)rs, rw, b.wfs.as<uint32_t>() + w0, b.len.as<uint32_t>(), b.off.as<uint64_t>(), b.bases.as<uint32_t>()};
            cw_result rres{r.cons.as<char>(), r.coff.as<uint64_t>() + w0, r.clen.as<uint32_t>() + w0, r.stat.as<uint8_t>() + w0, r.solid.as<uint32_t>(), r.soff.as<uint64_t>() + w0,
                           r.slen.as<uint32_t>() + w0};
            if (job_rc(cw_run_device_sync(eng, &run, &rres, st), j, "cw_run_device")) return j.rc;
            s0 = s1;
        }
        return CW_OK;
    }

    /* ---- re-assembly per read ---- (returns once the reads' lengths and every status are on the host) */
    int reassemble(const Shared& sh, Job& j, JobState& s) {
        const cw_driver_args& a = *sh.a;
        const uint32_t n_win = s.n_win, n_piles = s.n_piles;
        std::vector<uint64_t>& out_off = s.out_off;
        out_off.assign((size_t)n_piles + 1, 0);
        for (uint32_t i = 0; i < n_piles; ++i) out_off[i + 1] = out_off[i] + 2ull * sh.host_reads.read_len[j.sr[i].read] + 1024ull;
        if (job_rc(o.off.ensure((size_t)(n_piles + 1) * 8), j, "device memory (output)") || job_rc(o.buf.ensure(out_off[n_piles] + 16), j, "device memory (output)") ||
            job_rc(o.len.ensure((size_t)n_piles * 4), j, "device memory (output)") || job_rc(o.stat.ensure(n_piles), j, "device memory (output)"))
            return j.rc;
        if (job_hip(hipMemcpyAsync(o.off.p, out_off.data(), (size_t)(n_piles + 1) * 8, hipMemcpyHostToDevice, st), j, "H2D offsets") ||
            job_hip(hipMemsetAsync(o.len.p, 0, (size_t)n_piles * 4, st), j, "memset") || job_hip(hipMemsetAsync(o.stat.p, 0xFF, n_piles, st), j, "memset"))
            return j.rc;
        if (getenv("CW_DRIVER_TIMING")) { if (job_hip(hipStreamSynchronize(st), j, "sync")) return j.rc; s.t_stitch = now_ms(); }
        if (job_rc(cw_stitch_device(eng, &dev_reads, in.sr.as<cw_stitch_read>(), n_piles, in.pos.as<uint32_t>(), &s.batch, &s.res, a.window_size, a.window_overlap, sh.do_trim ? 1 : 0,
                                    o.buf.as<char>(), o.off.as<uint64_t>(), o.len.as<uint32_t>(), o.stat.as<uint8_t>(), st),
                   j, "cw_stitch_device"))
            return j.rc;
        s.h_len.resize(n_piles); s.h_st.resize(n_piles); s.h_wst.resize(n_win);
        if (job_hip(hipMemcpyAsync(s.h_len.data(), o.len.p, (size_t)n_piles * 4, hipMemcpyDeviceToHost, st), j, "D2H lengths") ||
            job_hip(hipMemcpyAsync(s.h_st.data(), o.stat.p, n_piles, hipMemcpyDeviceToHost, st), j, "D2H read status") ||
            job_hip(hipMemcpyAsync(s.h_wst.data(), r.stat.p, n_win, hipMemcpyDeviceToHost, st), j, "D2H window status") || job_hip(hipStreamSynchronize(st), j, "kernels"))
            return j.rc;
        if (s.t_stitch == 0) s.t_stitch = now_ms();
        return CW_OK;
    }

    /* a read whose re-assembly, or one of whose windows, exceeded a documented capacity is never silently different from the reference */
    int capacity_check(const Shared& sh, Job& j, JobState& s) {
        const uint32_t n_win = s.n_win, n_piles = s.n_piles;
        const std::vector<uint8_t>& h_st = s.h_st; const std::vector<uint8_t>& h_wst = s.h_wst;
        s.tainted.assign(n_piles, 0);
        std::string names;
        uint32_t n_bad = 0;
        for (uint32_t i = 0; i < n_piles; ++i) {
            bool bad = h_st[i] == CW_READ_CAPACITY;
            for (uint32_t w = j.sr[i].win_first; !bad && w < j.sr[i].win_first + j.sr[i].win_count; ++w) bad = h_wst[w] == CW_WIN_OVERFLOW;
            if (bad) {
                s.tainted[i] = 1;
                if (n_bad++ < 64) { names += names.empty() ? "" : ", "; names += cw_read_index_name(sh.index, j.sr[i].read); }
            }
        }
        if (n_bad) { /* say which capacity: the engine keeps a reason per window (CW_WHY_*, cw_device.h) */
            std::vector<uint32_t> wi((size_t)n_win * 16);
            uint32_t n_st = 0, hist[16] = {0};
            for (uint32_t i = 0; i < n_piles; ++i) n_st += h_st[i] == CW_READ_CAPACITY;
            if (cw_debug_win_info(eng, n_win, wi.data()) == CW_OK)
                for (uint32_t w = 0; w < n_win; ++w) if (h_wst[w] == CW_WIN_OVERFLOW) hist[wi[(size_t)w * 16 + 15] & 15u]++;
            names += " [";
            for (int q = 0; q < 16; ++q) if (hist[q]) names += "window reason " + std::to_string(q) + " x" + std::to_string(hist[q]) + "; ";
            names += std::to_string(n_st) + " read(s) beyond a re-assembly limit]";
        }
        if (n_bad && !sh.skip_on_capacity) {
            j.rc = CW_E_CAPACITY;
            j.err = "engine capacity exceeded for " + std::to_string(n_bad) + " read(s): " + names + (n_bad > 64 ? ", ..." : "") + " (CW_ON_CAPACITY=skip leaves them out)";
            return j.rc;
        }
        if (n_bad) fprintf(stderr, "[consent_amd] left out (engine capacity): %s%s\n", names.c_str(), n_bad > 64 ? ", ..." : "");
        return CW_OK;
    }

    /* only the corrected reads come back: one transfer of the output slots into pinned memory, then one string per read */
    int fetch_reads(Job& j, JobState& s) {
        const uint32_t n_piles = s.n_piles;
        const std::vector<uint64_t>& out_off = s.out_off;
        const std::vector<uint32_t>& h_len = s.h_len;
        uint64_t used_end = 0;
        for (uint32_t i = 0; i < n_piles; ++i)
            if (!s.tainted[i] && s.h_st[i] == CW_READ_OK && h_len[i]) used_end = out_off[i] + h_len[i];
        if (!used_end) return CW_OK;
        if (pin_cap < used_end) {
            if (pin) (void)hipHostFree(pin);
            pin = nullptr; pin_cap = 0;
            if (hipHostMalloc(&pin, used_end + used_end / 4, hipHostMallocDefault) != hipSuccess) { pin = nullptr; j.rc = CW_E_NOMEM; j.err = "pinned host memory"; return j.rc; }
            pin_cap = used_end + used_end / 4;
        }
        if (job_hip(hipMemcpyAsync(pin, o.buf.p, used_end, hipMemcpyDeviceToHost, st), j, "D2H reads") || job_hip(hipStreamSynchronize(st), j, "D2H reads")) return j.rc;
        for (uint32_t i = 0; i < n_piles; ++i)
            if (!s.tainted[i] && s.h_st[i] == CW_READ_OK && h_len[i]) j.out[i].assign((const char*)pin + out_off[i], h_len[i]);
        return CW_OK;
    }

    /* one job, start to end, on this worker's device: every phase returns CW_OK or the job's status (j.rc, j.err) */
    void process(const Shared& sh, Job& j) {
        JobState s;
        const uint32_t n_win = s.n_win = (uint32_t)j.wj.size(), n_piles = s.n_piles = (uint32_t)j.sr.size();
        j.out.assign(n_piles, std::string());
        j.device = device;
        if (n_win == 0 || n_piles == 0) return;
        if (sh.dry) { windows += n_win; reads += n_piles; jobs++; return; }
        const double t0 = now_ms();
        int rc = upload_job(j, s);
        if (rc == CW_OK) rc = extract(sh, j, s);
        const double t1 = now_ms();
        if (rc == CW_OK) rc = consensus(j, s);
        if (rc == CW_OK) rc = reassemble(sh, j, s);
        const double t2 = s.t_stitch;
        if (rc == CW_OK && getenv("CW_DRIVER_PROFILE")) print_job_profile(eng, j.seq, n_win);
        if (rc == CW_OK) rc = capacity_check(sh, j, s);
        if (rc == CW_OK) rc = fetch_reads(j, s);
        /* An error leaves process() while copies may still be queued on `st` whose host side are vectors of the JobState and of the Job:
           wait for the stream before they go out of scope (a late copy would write into freed memory -- exactly when the device misbehaves). */
        if (rc != CW_OK) { if (st) (void)hipStreamSynchronize(st); return; }
        const double t4 = now_ms();
        j.ms_extract = t1 - t0; j.ms_consensus = t2 - t1; j.ms_stitch = t4 - t2;
        windows += n_win; reads += n_piles; jobs++;
        ms_extract += j.ms_extract; ms_consensus += j.ms_consensus; ms_stitch += j.ms_stitch;
        if (const char* tv = getenv("CW_DRIVER_TIMING")) if (tv[0] == '2') /* inspection: when each job's phases ran, per worker */
            fprintf(stderr, "[job %llu] worker %p windows %u: start %.1f extract %.1f consensus %.1f (alloc %.1f) stitch %.1f ms\n", (unsigned long long)j.seq, (void*)this, n_win, t0 - sh.t_start, t1 - t0, t2 - t1, s.t_alloc, t4 - t2);
    }
};

void worker_main(Shared* sh, Worker* w) {
    for (;;) {
        Job* j = nullptr;
        {
            std::unique_lock<std::mutex> lk(sh->mu);
            sh->cv_work.wait(lk, [&] { return !sh->queue.empty() || sh->closed || sh->abort; });
            if (sh->abort || (sh->queue.empty() && sh->closed)) return;
            j = sh->queue.front();
            sh->queue.pop_front();
            sh->cv_room.notify_all();
        }
        w->process(*sh, *j);
        {
            std::lock_guard<std::mutex> lk(sh->mu);
            if (j->rc != CW_OK) sh->fail(j->rc, j->err);
            sh->finished[j->seq] = j;
            sh->cv_done.notify_all();
        }
    }
}

/* a worker's thread: engine and read set first, then jobs until the queue is closed and empty */
void worker_thread(Shared* sh, Worker* w, double* ms_init) {
    const double t0 = now_ms();
    const int irc = w->init(*sh);
    *ms_init = now_ms() - t0;
    if (irc != CW_OK) {
        std::lock_guard<std::mutex> lk(sh->mu);
        sh->fail(irc, "device " + std::to_string(w->device));
        return;
    }
    worker_main(sh, w);
}

bool write_all(int fd, const char* p, size_t n) {
    while (n) {
        const ssize_t k = write(fd, p, n);
        if (k < 0) return false;
        p += k; n -= (size_t)k;
    }
    return true;
}

/* writes finished jobs in submission order: the FASTA does not depend on which device took which job */
void emitter_main(Shared* sh, int out_fd, uint64_t* records, uint64_t* bases) {
    uint64_t next = 0;
    std::string buf;
    for (;;) {
        Job* j = nullptr;
        {
            std::unique_lock<std::mutex> lk(sh->mu);
            sh->cv_done.wait(lk, [&] { return sh->finished.count(next) || sh->abort || (sh->closed && next >= sh->n_jobs_total); });
            if (sh->abort) return;
            if (!sh->finished.count(next)) return; /* everything written */
            j = sh->finished[next];
            sh->finished.erase(next);
        }
        buf.clear();
        for (size_t i = 0; i < j->out.size(); ++i) {
            if (j->out[i].empty()) continue;
            buf += '>'; buf += cw_read_index_name(sh->index, j->sr[i].read); buf += '\n';
            buf += j->out[i]; buf += '\n';
            ++*records; *bases += j->out[i].size();
        }
        const bool ok = buf.empty() || write_all(out_fd, buf.data(), buf.size());
        delete j;
        ++next;
        if (!ok) {
            std::lock_guard<std::mutex> lk(sh->mu);
            sh->fail(CW_E_INTERNAL, "write to the output failed");
            return;
        }
    }
}

/* ---- producer: getNextReadPile -> getAlignmentWindowsPositions -> jobs ----
   Piles are read in PAF order on this thread (the reader parses blocks of the file ahead on its own threads, cw_hostio.cpp) a
   few hundred at a time; the window positions of one such round are computed on helper threads -- piles are independent -- while
   this thread already reads the next round; jobs are then put together in pile order, so their contents do not depend on the
   number of helpers.  One thread did all three before: 3 M windows/s, within 2x of what eight GPUs take. */
struct Producer {
    struct PileRec { uint32_t tpl, tpl_len, n, np; size_t ov_off; int rc; std::vector<uint32_t> wp; };
    struct Round { std::vector<PileRec> piles; std::vector<cw_overlap> ov; size_t used = 0; bool last = false; };
    Shared& sh;
    const cw_driver_args* a;
    const uint32_t per_job, max_batch; /* the plan's windows per job; what one engine call takes */
    cw_paf_reader* paf = nullptr;
    Round rounds[2];
    const size_t round_piles = 512, round_overlaps = 1u << 17;
    std::vector<cw_overlap> ov;
    Job* cur = nullptr;
    uint64_t job_cost_cap = 1ull << 26;
    unsigned n_help = 1;
    uint64_t n_piles = 0, n_windows = 0, n_overlaps = 0;
    double ms_parse = 0, ms_windows = 0;

    Producer(Shared& sh_, uint32_t per_job_, uint32_t max_batch_) : sh(sh_), a(sh_.a), per_job(per_job_), max_batch(max_batch_), ov(sh_.a->max_support ? sh_.a->max_support : 1) {
        n_help = std::thread::hardware_concurrency() / 2;
        if (n_help > 8) n_help = 8;
        if (const char* env = getenv("CW_PRODUCER_THREADS")) { const int v = atoi(env); if (v >= 1 && v <= 64) n_help = (unsigned)v; }
        if (n_help < 1) n_help = 1;
        if (const char* env = CW_AID_ENV("CW_JOB_COST_CAP")) { const long long v = atoll(env); if (v >= 1) job_cost_cap = (uint64_t)v; } /* test aid */
    }

    bool push_job() {
        if (cur->wj.empty()) return true;
        std::unique_lock<std::mutex> lk(sh.mu);
        cur->seq = sh.n_jobs_total;
        sh.cv_room.wait(lk, [&] { return sh.queue.size() < sh.queue_cap || sh.abort; });
        if (sh.abort) return false;
        sh.queue.push_back(cur);
        ++sh.n_jobs_total;
        sh.cv_work.notify_one();
        cur = new Job();
        return true;
    }
    /* stage 1 (this thread): the next piles of the file */
    int read_round(Round& r) {
        r.used = 0; r.ov.clear(); r.last = false;
        while (r.used < round_piles && r.ov.size() < round_overlaps) {
            uint32_t tpl = 0, tpl_len = 0, n = 0;
            const double tp0 = now_ms();
            const int prc = cw_paf_next_pile(paf, &tpl, &tpl_len, ov.data(), nullptr, (uint32_t)ov.size(), &n);
            ms_parse += now_ms() - tp0;
            if (prc != CW_OK) { fprintf(stderr, "[consent_amd] %s: %s (malformed line, a name missing from the read file, or a length that disagrees with it)\n", a->alignment_file, cw_strerror(prc)); return prc; }
            if (n == 0) { r.last = true; break; }
            if (tpl_len != sh.host_reads.read_len[tpl]) {
                fprintf(stderr, "[consent_amd] %s states length %u for %s, the read file has %u\n", a->alignment_file, tpl_len, cw_read_index_name(sh.index, tpl), sh.host_reads.read_len[tpl]);
                return CW_E_INVALID;
            }
            if (r.used == r.piles.size()) r.piles.emplace_back();
            PileRec& p = r.piles[r.used++];
            p.tpl = tpl; p.tpl_len = tpl_len; p.n = n; p.np = 0; p.rc = CW_OK; p.ov_off = r.ov.size();
            r.ov.insert(r.ov.end(), ov.begin(), ov.begin() + n);
        }
        return CW_OK;
    }
    /* stage 2 (helpers): window positions of every pile of a round */
    void positions(Round& r) {
        std::atomic<size_t> next{0};
        auto work = [&]() {
            for (;;) {
                const size_t i = next.fetch_add(1, std::memory_order_relaxed);
                if (i >= r.used) return;
                PileRec& p = r.piles[i];
                p.wp.resize(2 * ((size_t)p.tpl_len / (a->window_size - a->window_overlap) + 8));
                uint32_t np = 0;
                int wrc = cw_window_positions(p.tpl_len, r.ov.data() + p.ov_off, p.n, a->min_support, a->window_size, (int32_t)a->window_overlap, p.wp.data(), (uint32_t)(p.wp.size() / 2), &np);
                if (wrc == CW_E_CAPACITY) { p.wp.resize(2 * (size_t)np); wrc = cw_window_positions(p.tpl_len, r.ov.data() + p.ov_off, p.n, a->min_support, a->window_size, (int32_t)a->window_overlap, p.wp.data(), np, &np); }
                p.np = np; p.rc = wrc;
            }
        };
        const unsigned nt = (unsigned)std::min<size_t>(n_help, (r.used + 15) / 16);
        std::vector<std::thread> th;
        for (unsigned t = 1; t < nt; ++t) th.emplace_back(work);
        work();
        for (auto& t : th) t.join();
    }
    /* stage 3 (this thread): jobs, in pile order */
    int assemble(Round& r) {
        for (size_t i = 0; i < r.used; ++i) {
            PileRec& p = r.piles[i];
            if (p.rc != CW_OK) return p.rc;
            ++n_piles;
            const uint32_t np = p.np, n = p.n;
            if (np == 0) continue; /* processRead returns (readId, "") before anything else (CONSENT-correction.cpp:22-25) */
            /* (a read or contig with more windows than one engine call takes -- CW_MAX_BATCH_WINDOWS -- becomes a job of its own: the worker
               corrects it in several runs and re-assembles it once, Worker::process) */
            /* a job's extraction scratch is one descriptor per (window, overlap of its pile): polishing with -S 20000 looks at every
               overlap of the contig for every window (alignmentWindows.cpp:105), so jobs are also cut by that product -- 2^26
               descriptors = 1 GiB; only a single pile larger than that still makes a larger job (a read's windows are never split) */
            if (!cur->wj.empty() && (cur->wj.size() + np > max_batch || cur->cost + (uint64_t)np * (n + 1) > job_cost_cap) && !push_job()) return CW_E_INTERNAL;
            cw_stitch_read sr_{p.tpl, (uint32_t)cur->wj.size(), np};
            const uint32_t ovl_first = (uint32_t)cur->ovl.size();
            cur->ovl.insert(cur->ovl.end(), r.ov.begin() + (ptrdiff_t)p.ov_off, r.ov.begin() + (ptrdiff_t)(p.ov_off + n));
            for (uint32_t w = 0; w < np; ++w) {
                cur->wj.push_back(cw_window_job{p.tpl, p.wp[2 * w], p.wp[2 * w + 1], ovl_first, n});
                cur->win_pos.push_back(p.wp[2 * w]); cur->win_pos.push_back(p.wp[2 * w + 1]);
            }
            cur->sr.push_back(sr_);
            cur->cost += (uint64_t)np * (n + 1);
            n_windows += np; n_overlaps += n;
            if (cur->wj.size() >= per_job && !push_job()) return CW_E_INTERNAL;
        }
        return CW_OK;
    }
    /* the whole file; CW_OK also when a worker failed (its error is the run's) */
    int run() {
        int rc = cw_paf_open(a->alignment_file, sh.index, a->max_support, &paf);
        if (rc != CW_OK) { fprintf(stderr, "[consent_amd] cannot open %s\n", a->alignment_file); return rc; }
        cur = new Job();
        int k = 0;
        rc = read_round(rounds[0]);
        while (rc == CW_OK) {
            Round& r = rounds[k];
            int rrc = CW_OK;
            const double tw0 = now_ms();
            if (r.last && r.used == 0) break;
            if (r.last) positions(r); /* nothing left to read beside it */
            else {
                std::thread helper([&] { positions(r); });
                rrc = read_round(rounds[k ^ 1]);
                helper.join();
            }
            ms_windows += now_ms() - tw0; /* includes the reading that ran beside it */
            rc = assemble(r);
            if (rc == CW_E_INTERNAL && sh.abort) { rc = CW_OK; break; } /* a worker failed: its error is reported below */
            if (rc == CW_OK) rc = rrc;
            if (r.last) break;
            k ^= 1;
        }
        if (rc == CW_OK && !sh.abort) push_job();
        delete cur;
        cw_paf_close(paf);
        return rc;
    }
};

/* ---- indexReads (+ the proof file into the same index) ----; *tpl_bases = bases of the templates (the sequences of reads_file: every one of them may be a pile's query) */
int index_reads(Shared& sh, uint64_t* tpl_bases, double* t_indexed) {
    const cw_driver_args* a = sh.a;
    /* the HIP runtime takes ~0.1 s to start (first call of the process): let it start while the reads are indexed */
    const bool dry = sh.dry;
    struct Joiner { std::thread t; ~Joiner() { if (t.joinable()) t.join(); } } hip_warm{std::thread([dry] { if (dry || CW_AID_ENV("CW_NO_WARM")) return; int n = 0; (void)hipGetDeviceCount(&n); if (n > 0) (void)hipFree(nullptr); })};
    int rc = cw_index_reads(a->reads_file, &sh.index);
    if (rc != CW_OK) { fprintf(stderr, "[consent_amd] cannot index %s: %s\n", a->reads_file, cw_strerror(rc)); return rc; }
    {
        cw_read_set v0; uint64_t w0 = 0;
        cw_read_index_view(sh.index, &v0, &w0);
        for (uint32_t i = 0; i < v0.n_reads; ++i) *tpl_bases += v0.read_len[i];
    }
    if (a->proof_file && a->proof_file[0] && (rc = cw_index_reads_append(sh.index, a->proof_file)) != CW_OK) {
        fprintf(stderr, "[consent_amd] cannot index %s: %s\n", a->proof_file, cw_strerror(rc));
        return rc;
    }
    cw_read_index_view(sh.index, &sh.host_reads, &sh.read_words);
    *t_indexed = now_ms(); /* (the runtime's start is waited for after this: hip_warm's destructor) */
    return CW_OK;
}

/* ---- devices: explicit list, or CW_DEVICES="0,1,..." (an id may repeat: several engines on one GPU), or the first
        min(nb_threads, device count) devices ----; workers, job size and queue: cw_driver_plan.h, from these and the switches read here */
int plan_run(const Shared& sh, uint64_t tpl_bases, DriverPlan* plan, uint32_t* max_batch) {
    const cw_driver_args* a = sh.a;
    DriverPlanInput in;
    in.a = a; in.tpl_bases = tpl_bases; in.dry = sh.dry;
    if (a->devices && a->n_devices > 0) in.devs.assign(a->devices, a->devices + a->n_devices);
    else if (const char* env = getenv("CW_DEVICES")) {
        for (const char* p = env; *p;) { char* e = nullptr; const long v = strtol(p, &e, 10); if (e == p) break; in.devs.push_back((int)v); p = *e == ',' ? e + 1 : e; }
    }
    if (!sh.dry && (hipGetDeviceCount(&in.hip_devices) != hipSuccess || in.hip_devices <= 0)) { fprintf(stderr, "[consent_amd] no HIP device: the engine has no CPU path\n"); return CW_E_NO_DEVICE; }
    if (!sh.dry) if (const char* env = CW_AID_ENV("CW_VIRTUAL_DEVICES")) in.virtual_devices = atoi(env);
    if (const char* env = getenv("CW_WORKERS_PER_DEVICE")) in.workers_per_device = atoi(env);
    if (const char* env = CW_AID_ENV("CW_JOB_WINDOWS")) in.job_windows = atol(env);
    *max_batch = in.max_batch = cw_plan_max_batch_windows(a->mer_size, a->window_size);
    return cw_driver_plan(in, plan);
}

/* Engines and read-set uploads start on the worker threads themselves (all devices at once) while the calling thread already parses the
   alignments: creating two engines with their scratch takes 0.2-0.3 s, during which the producer fills the queue */
void start_workers(Shared& sh, const DriverPlan& plan, std::vector<Worker>& workers, std::vector<double>& ms_init, std::vector<std::thread>& threads) {
    for (size_t i = 0; i < workers.size(); ++i) {
        workers[i].device = plan.workers[i].device;
        workers[i].phys = plan.workers[i].phys;
        if (plan.workers[i].owner >= 0) workers[i].owner = &workers[(size_t)plan.workers[i].owner];
    }
    {   /* one future per owner, shared by its borrowers */
        std::vector<std::shared_future<int>> fut(workers.size());
        for (size_t i = 0; i < workers.size(); ++i) if (!workers[i].owner) fut[i] = workers[i].reads_ready.get_future().share();
        for (size_t i = 0; i < workers.size(); ++i) if (workers[i].owner) workers[i].reads_of_owner = fut[(size_t)(workers[i].owner - &workers[0])];
    }
    sh.queue_cap = plan.queue_cap;
    for (size_t i = 0; i < workers.size(); ++i) threads.emplace_back(worker_thread, &sh, &workers[i], &ms_init[i]);
}

/* the producer is done (rc: how it ended): close the queue, let the workers and the emitter finish, drop what an aborted run left behind */
void shut_down(Shared& sh, int rc, std::vector<std::thread>& threads, std::thread& emitter) {
    {
        std::lock_guard<std::mutex> lk(sh.mu);
        sh.closed = true;
        if (rc != CW_OK) sh.fail(rc, "reading the alignments");
        sh.cv_work.notify_all(); sh.cv_done.notify_all(); sh.cv_room.notify_all();
    }
    for (auto& t : threads) t.join();
    {
        std::lock_guard<std::mutex> lk(sh.mu);
        sh.cv_done.notify_all();
    }
    emitter.join();
    for (auto& kv : sh.finished) delete kv.second;
    for (Job* j : sh.queue) delete j;
}

struct RunTimes { double indexed, produced, end; std::vector<double> ms_init; }; /* now_ms() at the ends of the steps; how long each worker's init took */

void report(const Shared& sh, const DriverPlan& plan, const Producer& prod, const std::vector<Worker>& workers, const RunTimes& t, uint64_t records, uint64_t bases_out, cw_driver_stats* stats) {
    const double t_begin = sh.t_start, t_indexed = t.indexed, t_end = t.end;
    if (stats) {
        stats->n_devices = (uint32_t)workers.size();
        stats->piles = prod.n_piles; stats->windows = prod.n_windows; stats->overlaps = prod.n_overlaps; stats->jobs = sh.n_jobs_total;
        stats->records = records; stats->bases_out = bases_out;
        stats->ms_index = t_indexed - t_begin; stats->ms_total = t_end - t_begin;
        for (size_t i = 0; i < workers.size() && i < 16; ++i) {
            stats->dev_windows[i] = workers[i].windows;
            stats->dev_ms_extract[i] = workers[i].ms_extract; stats->dev_ms_consensus[i] = workers[i].ms_consensus; stats->dev_ms_stitch[i] = workers[i].ms_stitch;
        }
    }
    if (!getenv("CW_DRIVER_STATS")) return; /* counters on stderr; stdout stays pure FASTA */
    fprintf(stderr, "{\"dry\": %s, \"producer_threads\": %u, \"ms_producer\": %.1f, \"workers\": %zu, \"workers_per_device\": %zu, \"windows_per_job\": %u, \"piles\": %llu, \"windows\": %llu, \"jobs\": %llu, \"records\": %llu, \"bases_out\": %llu, \"ms_index\": %.1f, \"ms_engines\": %.1f, \"ms_paf_parse\": %.1f, \"ms_window_positions\": %.1f, \"ms_total\": %.1f, \"windows_per_s\": %.1f, \"per_device\": [",
            sh.dry ? "true" : "false", prod.n_help, t.produced - t_indexed, workers.size(), plan.workers_per_device, plan.windows_per_job, (unsigned long long)prod.n_piles, (unsigned long long)prod.n_windows, (unsigned long long)sh.n_jobs_total, (unsigned long long)records, (unsigned long long)bases_out,
            t_indexed - t_begin, *std::max_element(t.ms_init.begin(), t.ms_init.end()), prod.ms_parse, prod.ms_windows, t_end - t_begin, prod.n_windows / ((t_end - t_indexed) * 1e-3 + 1e-9));
    for (size_t i = 0; i < workers.size(); ++i)
        fprintf(stderr, "%s{\"device\": %d, \"windows\": %llu, \"jobs\": %llu, \"ms_extract\": %.1f, \"ms_consensus\": %.1f, \"ms_stitch\": %.1f}", i ? ", " : "", workers[i].device,
                (unsigned long long)workers[i].windows, (unsigned long long)workers[i].jobs, workers[i].ms_extract, workers[i].ms_consensus, workers[i].ms_stitch);
    fprintf(stderr, "]}\n");
}

} // namespace

extern "C" int cw_run_correction(const cw_driver_args* a, int out_fd, cw_driver_stats* stats) {
    if (stats) memset(stats, 0, sizeof(*stats));
    if (!a || !a->alignment_file || !a->reads_file || out_fd < 0) return CW_E_INVALID;
    if (a->window_size == 0 || a->window_overlap >= a->window_size || a->mer_size < 2 || a->mer_size > 16 || a->solid_thresh < 1 || a->max_msa < 1 || a->max_support < 1) return CW_E_INVALID;
    Shared sh;
    sh.a = a;
    sh.t_start = now_ms();
    sh.do_trim = !a->polishing && !(a->proof_file && a->proof_file[0]); /* CONSENT-correction.cpp:17,69-73; CONSENT-polishing.cpp:19 */
    if (const char* oc = getenv("CW_ON_CAPACITY")) sh.skip_on_capacity = strcmp(oc, "skip") == 0;
    /* GPU_MAX_HW_QUEUES (hardware queues HIP spreads a process's streams over, default 4, read when the runtime starts) is the HOST
       PROCESS's business: bin/CONSENT-* set it to 12 in main() before anything touches HIP, consent_amd/pipeline.py before the library is
       loaded; an embedding application does the same (include/consent_amd.h "Threading").  A library call does not change its caller's
       environment. */
    if (const char* dr = CW_AID_ENV("CW_DRIVER_DRY")) sh.dry = dr[0] && dr[0] != '0';

    uint64_t tpl_bases = 0;
    RunTimes t;
    DriverPlan plan;
    uint32_t max_batch = 0;
    int rc = index_reads(sh, &tpl_bases, &t.indexed);
    if (rc == CW_OK) rc = plan_run(sh, tpl_bases, &plan, &max_batch);
    if (rc != CW_OK) { cw_read_index_free(sh.index); return rc; }

    std::vector<Worker> workers(plan.workers.size());
    t.ms_init.assign(workers.size(), 0.0);
    uint64_t records = 0, bases_out = 0;
    std::vector<std::thread> threads;
    Producer prod(sh, plan.windows_per_job, max_batch);
    start_workers(sh, plan, workers, t.ms_init, threads);
    std::thread emitter(emitter_main, &sh, out_fd, &records, &bases_out);

    rc = prod.run();
    t.produced = now_ms();
    shut_down(sh, rc, threads, emitter);
    t.end = now_ms();
    report(sh, plan, prod, workers, t, records, bases_out, stats);
    for (auto& w : workers) w.close();
    cw_read_index_free(sh.index);
    if (sh.first_error != CW_OK) fprintf(stderr, "[consent_amd] %s: %s\n", sh.first_error_msg.c_str(), cw_strerror(sh.first_error));
    return sh.first_error;
}
