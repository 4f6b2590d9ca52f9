// pt_sync.hpp — the owners of the frame loop's synchronisation (private): an event that knows whether it was recorded,
// a stream, the version ring of a resource that changes under frames in flight, the pinned staging ring of its updates,
// the timed events of a pass and of a render's launches.  The only file of the library that creates or destroys an
// event or a stream.  Only the HIP runtime API: tests/sync_rings_main.cpp drives them on a CPU against fakes of it.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "pt_error.hpp"

namespace ppt
{

struct NoCopy
{
    NoCopy() = default;
    NoCopy(const NoCopy &) = delete;
    NoCopy &operator=(const NoCopy &) = delete;
};

// One event without timing, made by its first record and destroyed with its owner.  Waiting for a fence that was
// never recorded does nothing.
class Fence : NoCopy
{
  public:
    ~Fence() { if (ev) (void)hipEventDestroy(ev); }
    int record(hipStream_t s)
    {
        if (!ev) PPT_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        PPT_HIP(hipEventRecord(ev, s));
        recorded = true;
        return PROSPER_PT_OK;
    }
    int wait(hipStream_t s) const
    {
        if (recorded) PPT_HIP(hipStreamWaitEvent(s, ev, 0));
        return PROSPER_PT_OK;
    }
    int host_wait() const
    {
        if (recorded) PPT_HIP(hipEventSynchronize(ev));
        return PROSPER_PT_OK;
    }
    bool passed() const { return !recorded || hipEventQuery(ev) == hipSuccess; }
    // for a wait that someone else enqueues (pt_kernels.hpp WavefrontChains): nullptr if there is nothing to wait for
    hipEvent_t event() const { return recorded ? ev : nullptr; }

  private:
    hipEvent_t ev = nullptr;
    bool recorded = false;
};

// One non-blocking stream, destroyed with its owner.  A create() that failed leaves it empty.
class Stream : NoCopy
{
  public:
    ~Stream() { if (s) (void)hipStreamDestroy(s); }
    int create()
    {
        if (!s) PPT_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        return PROSPER_PT_OK;
    }
    hipStream_t get() const { return s; }

  private:
    hipStream_t s = nullptr;
};

// Pinned host memory, freed with its owner.
template <class T> struct Pinned : NoCopy
{
    T *ptr = nullptr;
    size_t bytes = 0;
    ~Pinned() { if (ptr) (void)hipHostFree(ptr); }
    // (what it held before is freed first; on a failure it holds nothing)
    int allocate(size_t n)
    {
        bytes = 0;
        if (ptr) PPT_HIP(hipHostFree(ptr));
        ptr = nullptr;
        PPT_HIP(hipHostMalloc((void **)&ptr, n, hipHostMallocDefault));
        bytes = n;
        return PROSPER_PT_OK;
    }
};

// N device versions of a resource.  Renders read version `cur`; an update is written into next() by the next render's
// own chain while the frames in flight go on reading theirs: wait_free(next) on that chain's stream, enqueue the
// writes, and commit(next) once EVERY enqueue has succeeded - on a failure `cur` stays and the update stays pending.
// Versions below First are written once, by the upload, and never again.
template <uint32_t N, uint32_t First = 0> class VersionRing
{
  public:
    uint32_t cur = 0;
    uint32_t next() const { return cur + 1u < N ? cur + 1u : First; }
    // `s` waits for the last readers of version v
    int wait_free(uint32_t v, hipStream_t s) const { return freed[v].wait(s); }
    // ... of every version (a rewrite of something that exists once, for all versions)
    int wait_all_free(hipStream_t s) const
    {
        for (const Fence &f : freed)
            if (const int rc = f.wait(s)) return rc;
        return PROSPER_PT_OK;
    }
    void commit(uint32_t v) { cur = v; }
    // Version `cur` is free again behind what `s` holds now.  One fence per version: a reader on ANOTHER stream than
    // the previous reader's first waits for that one, so the newest record always stands for every reader so far.
    int mark_read(hipStream_t s)
    {
        if (reader[cur] != s)
            if (const int rc = freed[cur].wait(s)) return rc;
        if (const int rc = freed[cur].record(s)) return rc;
        reader[cur] = s;
        return PROSPER_PT_OK;
    }

  private:
    Fence freed[N];
    hipStream_t reader[N] = {}; // the stream freed[] was last recorded on
};

// Pinned staging buffers per kind of update (transforms, lights, material tables): an update's copy is enqueued at the
// head of the next render's chain, i.e. BEHIND the frames in flight; with two buffers the update after next may wait on
// the host for that copy - with one buffer more than frames in flight it never does.
constexpr uint32_t kStagingBuffers = 4;

template <class T> class StagingRing
{
  public:
    // The buffer (allocated with `bytes` at its first use) the caller fills with an update.  `pending`: the previous
    // update was never consumed (or its copy never enqueued) and is replaced in its own buffer; otherwise the ring moves
    // on.  The host waits only for a copy out of that buffer that is still queued (the one of four updates ago).
    int acquire(size_t bytes, bool pending, T **out)
    {
        pending = pending || held;
        const uint32_t k = pending ? index : following;
        if (!pending) following = (following + 1u) % kStagingBuffers;
        if (!buffers[k].ptr)
            if (const int rc = buffers[k].allocate(bytes)) return rc;
        if (queued[k])
            if (const int rc = copied[k].host_wait()) return rc;
        queued[k] = false;
        index = k;
        held = true;
        *out = buffers[k].ptr;
        return PROSPER_PT_OK;
    }
    // the buffer of the last acquire
    T *pending_buffer() const { return buffers[index].ptr; }
    // the copy out of it has been enqueued on `s`
    int copy_enqueued(hipStream_t s)
    {
        if (const int rc = copied[index].record(s)) return rc;
        queued[index] = true;
        held = false;
        return PROSPER_PT_OK;
    }

  private:
    Pinned<T> buffers[kStagingBuffers];
    Fence copied[kStagingBuffers];
    bool queued[kStagingBuffers] = {}; // copied[k] was recorded and not waited for since
    uint32_t following = 0, index = 0;
    bool held = false; // acquired, and the copy not enqueued yet
};

// N events with timing, made by create() (again after a failure: only the missing ones) and destroyed with their owner.
template <uint32_t N> struct TimedEvents : NoCopy
{
    hipEvent_t events[N] = {};
    ~TimedEvents()
    {
        for (hipEvent_t e : events)
            if (e) (void)hipEventDestroy(e);
    }
    int create()
    {
        for (hipEvent_t &e : events)
            if (!e) PPT_HIP(hipEventCreate(&e));
        return PROSPER_PT_OK;
    }
};

// The timed events around the N stages of a pass (IBL, depth of field, bloom, the multi-GPU gather).
template <uint32_t N> struct StageEvents : TimedEvents<N + 1>
{
    bool created() const { return this->events[N] != nullptr; }
    // waits for the last stage; ms[k] = what stage k took
    int elapsed(float *ms) const
    {
        PPT_HIP(hipEventSynchronize(this->events[N]));
        for (uint32_t k = 0; k < N; ++k) PPT_HIP(hipEventElapsedTime(&ms[k], this->events[k], this->events[k + 1u]));
        return PROSPER_PT_OK;
    }
};

// Per-launch timestamps of a render (prosper_pt_set_kernel_timing): one event before every launch of a stream, one after
// the last; interval i belongs to stage[i].  A launcher that is handed no timeline (nullptr) runs untimed.
constexpr uint32_t kMaxTimedLaunches = 96;
class LaunchTimeline : TimedEvents<kMaxTimedLaunches + 1>
{
  public:
    using TimedEvents::create;
    void begin() { count = 0; }
    // (launches beyond the capacity go untimed)
    void mark(uint32_t st, hipStream_t stream)
    {
        if (count < kMaxTimedLaunches)
        {
            (void)hipEventRecord(events[count], stream);
            stage[count] = st;
            ++count;
        }
    }
    void close(hipStream_t stream) { (void)hipEventRecord(events[count], stream); }
    uint32_t intervals() const { return count; }
    // the host waits for the closing event
    int wait() const
    {
        PPT_HIP(hipEventSynchronize(events[count]));
        return PROSPER_PT_OK;
    }
    // every interval into its stage's milliseconds and launch count, and into *total
    int add_to(float *stageMs, uint32_t *stageLaunches, float *total) const
    {
        for (uint32_t i = 0; i < count; ++i)
        {
            float ms = 0.0f;
            PPT_HIP(hipEventElapsedTime(&ms, events[i], events[i + 1u]));
            stageMs[stage[i]] += ms;
            stageLaunches[stage[i]] += 1;
            *total += ms;
        }
        return PROSPER_PT_OK;
    }

  private:
    uint32_t stage[kMaxTimedLaunches] = {};
    uint32_t count = 0; // intervals recorded so far (events used = count + 1 once closed)
};

} // namespace ppt
