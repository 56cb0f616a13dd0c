/* cw_driver_plan.h -- the native driver's job plan: which workers serve which device, how many windows make a job and how deep the job queue is.
   Host arithmetic only, no call into the HIP runtime and no getenv (cw_driver.cpp reads the switches and passes their values): cw_run_correction starts its
   workers and cuts its jobs by it, and tests/test_driver_dry.py pins its numbers (tests/golden/driver_plan.json). */
#ifndef CW_DRIVER_PLAN_H
#define CW_DRIVER_PLAN_H

#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/consent_amd.h"

struct DriverPlanInput {
    const cw_driver_args* a = nullptr;
    uint64_t tpl_bases = 0;        /* bases of the templates (the sequences of reads_file: every one of them may be a pile's query): sizes the jobs */
    bool dry = false;              /* CW_DRIVER_DRY: no device is asked; as many "devices" as were asked for stand in */
    int hip_devices = 0;           /* hipGetDeviceCount (not looked at in a dry run) */
    std::vector<int> devs;         /* the explicit list or CW_DEVICES; empty = the first min(nb_threads, device count) devices */
    uint32_t max_batch = 0;        /* cw_plan_max_batch_windows: what cw_max_batch_windows will say of the workers' engines */
    int workers_per_device = 0;    /* CW_WORKERS_PER_DEVICE; 0 = not set */
    long job_windows = 0;          /* CW_JOB_WINDOWS (test aid: jobs of a few windows, so that a small data set reaches every worker); 0 = not set */
    int virtual_devices = 0;       /* CW_VIRTUAL_DEVICES (test aid, below); 0 = not set */
};

struct DriverPlan {
    struct WorkerSlot {
        int device; /* the device this worker serves: read-set ownership, statistics */
        int phys;   /* the HIP device behind it (== device, except under the test aid CW_VIRTUAL_DEVICES: several logical devices on one GPU) */
        int owner;  /* the earlier worker on the same device whose copy of the read set this one borrows; -1 = it uploads (and owns) the copy */
    };
    std::vector<WorkerSlot> workers;
    size_t distinct_devs = 0, workers_per_device = 0; /* (workers / distinct devices: what the statistics line reports) */
    uint64_t est_windows = 0;
    uint32_t windows_per_job = 0;
    size_t queue_cap = 0;
};

/* CW_OK, or CW_E_INVALID for a device id outside the devices there are */
static inline int cw_driver_plan(const DriverPlanInput& in, DriverPlan* p) {
    const cw_driver_args* a = in.a;
    std::vector<int> devs = in.devs;
    int n_dev = in.hip_devices;
    if (in.dry) { n_dev = a->nb_threads < 1 ? 1 : (int)a->nb_threads; for (int d : devs) n_dev = d + 1 > n_dev ? d + 1 : n_dev; } /* as many "devices" as were asked for */
    /* test aid (-DCW_TEST_AIDS build only): CW_VIRTUAL_DEVICES=8 makes the one GPU of a test box eight logical devices -- eight read-set uploads,
       the workers, job size and queue an 8-GPU node gets (tests/test_gpu_driver.py); logical device v runs on HIP device v % (physical count) */
    const int n_phys = n_dev > 0 ? n_dev : 1;
    if (!in.dry && in.virtual_devices >= 1 && in.virtual_devices <= 64) n_dev = in.virtual_devices;
    /* The number of windows is not known before the alignments are read, but it is close to template bases / (window size - overlap) */
    p->est_windows = in.tpl_bases / (a->window_size - a->window_overlap) + 1;
    if (devs.empty()) {
        /* two workers (engine + buffers each) per device: while one job is in its re-assembly -- one wave per read, the longest read sets
           the time, most of the GPU idle -- the other worker's consensus kernels run (measured on one GPU: 717 -> 550 ms for 112 k windows) */
        const int want = a->nb_threads < 1 ? 1 : (int)a->nb_threads;
        /* A run that gives a device fewer than ~1e5 windows (the E. coli-scale set on eight GPUs: 4e4 each) is cut into jobs of a few
           thousand windows, whose fixed costs -- the longest POA task, the longest read of the re-assembly, the synchronisation points of a
           run -- no longer hide behind one other job: four workers per device then (measured on one GPU with jobs of 5000 windows:
           1.97e5 windows/s with two workers, 2.36e5 with three, 2.77e5 with four; with jobs of 32768: 3.3e5 / 2.8e5 / 2.8e5) */
        const uint64_t est_per_dev = p->est_windows / (uint64_t)(n_dev < want ? n_dev : want);
        /* round 6: two workers also for a small per-device load (four from round 4 on, when such a run was cut into jobs of ~5000 windows).  With three larger jobs
           per device (below) two workers are as fast (a device's 4.2e4 windows: 0.134-0.138 s with two workers on two or three jobs, 0.133-0.134 s with four
           on two or four; profiles/r06_job_size_sweep.txt) and set up half the engines: an engine's scratch is ~10 GB, and obtaining that much new device
           memory is where a fresh process can stall for a second or more (hipMalloc: 0.2 ms or 0.5-1.9 s a call) */
        int per_dev = 2; /* (whatever the input: a run of fewer windows than the 4096-window floor is one job, and one of its device's two workers gets none) */
        if (est_per_dev >= 1000000ull) per_dev = 3;
        if (in.workers_per_device >= 1 && in.workers_per_device <= 8) per_dev = in.workers_per_device;
        for (int k = 0; k < per_dev; ++k) for (int d = 0; d < n_dev && d < want; ++d) devs.push_back(d);
    }
    for (int d : devs) if (d < 0 || d >= n_dev) return CW_E_INVALID;
    /* The 2-bit read set is uploaded once per DEVICE: the first worker on a device owns the copy, the others on that device borrow it */
    p->workers.clear();
    for (size_t i = 0; i < devs.size(); ++i) {
        p->workers.push_back({devs[i], devs[i] % n_phys, -1});
        for (size_t o = 0; o < i; ++o)
            if (p->workers[o].owner < 0 && p->workers[o].device == devs[i]) { p->workers[i].owner = (int)o; break; }
    }
    { std::vector<int> distinct(devs); std::sort(distinct.begin(), distinct.end()); distinct.erase(std::unique(distinct.begin(), distinct.end()), distinct.end()); p->distinct_devs = distinct.size(); }
    p->workers_per_device = devs.size() / std::max<size_t>(1, p->distinct_devs);
    p->queue_cap = 2 * devs.size() + 1;

    /* Windows per job.  The caller's figure, else 32768 -- unless the run is too short for that many workers: a job is the unit the workers
       share, and with fewer than about eight jobs per device the last ones leave most engines idle (the E. coli-scale set is 3.2e5 windows:
       ten jobs of 32768 for an 8-GPU node); floor 4096 windows (below that a job no longer fills a GPU). */
    uint32_t per_job = a->windows_per_batch ? a->windows_per_batch : 32768u;
    if (per_job > in.max_batch) per_job = in.max_batch;
    if (!a->windows_per_batch && p->distinct_devs) {
        /* jobs per device.  Eight (four per worker with two workers) while a device gets 1e5 windows or more; THREE below that (round 6): a device that gets
           4e4 windows -- the E. coli-scale set on eight GPUs -- ran its nine jobs of 5 200 windows on four workers in 0.234 s, and four jobs of 10 400 on the
           same four workers in 0.134 s (two jobs of 20 800 on two: 0.138; tools/job_size_model.py JSM_MODE=sweep, profiles/r06_job_size_sweep.txt): a job's
           fixed costs -- its longest POA task, its longest read, its launches and synchronisation points -- are paid once per job and worker, and small
           jobs do not fill the GPU while they are paid */
        const uint64_t jobs_per_dev = p->est_windows / p->distinct_devs < 100000ull ? 3ull : 8ull;
        const uint64_t want = p->est_windows / (jobs_per_dev * p->distinct_devs) + 1;
        if (want < per_job) per_job = (uint32_t)(want < 4096 ? 4096 : want);
    }
    if (in.job_windows >= 1 && in.job_windows <= (long)in.max_batch) per_job = (uint32_t)in.job_windows;
    p->windows_per_job = per_job;
    return CW_OK;
}

#endif
