// sync_rings_main.cpp — the fence, stream, version ring, staging ring and launch timeline of prosper_amd/csrc/pt_sync.hpp
// on a CPU, against fakes of the HIP entry points the header calls: every fake appends to a call log and can be told to
// fail once.  Built and
// run by tests/test_sync_rings.py (host compiler, no HIP runtime linked, AddressSanitizer + UBSan).  Exit status 0: every
// check held.
#include "pt_sync.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <string>
#include <vector>

using namespace ppt;

namespace
{

struct Call
{
    std::string op;
    const void *event, *stream;
};
std::vector<Call> g_log;
std::string g_failOnce; // the next call of this entry point fails (once)
uint32_t g_failAt = 0;  // ... or the g_failAt-th hipEventCreate from now on does (once)
std::set<void *> g_liveEvents, g_livePinned, g_liveStreams;
std::map<const void *, float> g_msFrom; // what hipEventElapsedTime reports for an interval that starts at this event
int g_eventsCreated = 0, g_eventsDestroyed = 0, g_pinnedAllocated = 0, g_pinnedFreed = 0;
int g_streamsCreated = 0, g_streamsDestroyed = 0;
std::string g_lastError;
int g_failures = 0;

hipError_t enter(const char *op, const void *event = nullptr, const void *stream = nullptr)
{
    if (g_failOnce == op)
    {
        g_failOnce.clear();
        g_log.push_back({std::string(op) + "!", event, stream});
        return hipErrorUnknown;
    }
    g_log.push_back({op, event, stream});
    return hipSuccess;
}

size_t count(const char *op, size_t from = 0, const void *event = nullptr)
{
    size_t n = 0;
    for (size_t i = from; i < g_log.size(); ++i)
        if (g_log[i].op == op && (!event || g_log[i].event == event)) ++n;
    return n;
}

#define CHECK(cond)                                                                                                    \
    do                                                                                                                 \
    {                                                                                                                  \
        if (!(cond))                                                                                                   \
        {                                                                                                              \
            std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond);                              \
            ++g_failures;                                                                                              \
        }                                                                                                              \
    } while (0)

hipStream_t stream(uintptr_t n) { return reinterpret_cast<hipStream_t>(n << 4); } // (never dereferenced)

} // namespace

int ppt::fail(int code, const std::string &msg)
{
    g_lastError = msg;
    return code;
}

extern "C" {

const char *hipGetErrorString(hipError_t) { return "fake failure"; }
hipError_t hipEventCreateWithFlags(hipEvent_t *event, unsigned flags)
{
    if (flags != hipEventDisableTiming) return hipErrorInvalidValue;
    const hipError_t e = enter("create");
    if (e != hipSuccess) return e;
    *event = static_cast<hipEvent_t>(std::malloc(1)); // (a heap block each: ASan sees a leak or a second destroy)
    g_liveEvents.insert(*event);
    g_log.back().event = *event;
    ++g_eventsCreated;
    return hipSuccess;
}
hipError_t hipEventCreate(hipEvent_t *event)
{
    if (g_failAt && --g_failAt == 0) g_failOnce = "create_timed";
    const hipError_t e = enter("create_timed");
    if (e != hipSuccess) return e;
    *event = static_cast<hipEvent_t>(std::malloc(1));
    g_liveEvents.insert(*event);
    g_log.back().event = *event;
    ++g_eventsCreated;
    return hipSuccess;
}
hipError_t hipEventElapsedTime(float *ms, hipEvent_t start, hipEvent_t stop)
{
    if (!g_liveEvents.count(start) || !g_liveEvents.count(stop)) return hipErrorInvalidHandle;
    const hipError_t e = enter("elapsed", start, stop); // (the log's `stream` holds the closing event)
    if (e == hipSuccess) *ms = g_msFrom.count(start) ? g_msFrom[start] : 0.0f;
    return e;
}
hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned flags)
{
    if (flags != hipStreamNonBlocking) return hipErrorInvalidValue;
    const hipError_t e = enter("stream_create");
    if (e != hipSuccess) return e;
    *s = static_cast<hipStream_t>(std::malloc(1));
    g_liveStreams.insert(*s);
    g_log.back().stream = *s;
    ++g_streamsCreated;
    return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t s)
{
    if (!g_liveStreams.erase(s)) return hipErrorInvalidHandle;
    ++g_streamsDestroyed;
    std::free(s);
    return enter("stream_destroy", nullptr, s);
}
hipError_t hipEventDestroy(hipEvent_t event)
{
    if (!g_liveEvents.erase(event)) return hipErrorInvalidHandle;
    ++g_eventsDestroyed;
    std::free(event);
    return enter("destroy", event);
}
hipError_t hipEventRecord(hipEvent_t event, hipStream_t s) { return g_liveEvents.count(event) ? enter("record", event, s) : hipErrorInvalidHandle; }
hipError_t hipEventSynchronize(hipEvent_t event) { return g_liveEvents.count(event) ? enter("host_wait", event) : hipErrorInvalidHandle; }
hipError_t hipEventQuery(hipEvent_t event) { return g_liveEvents.count(event) ? enter("query", event) : hipErrorInvalidHandle; }
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t event, unsigned int) { return g_liveEvents.count(event) ? enter("wait", event, s) : hipErrorInvalidHandle; }
hipError_t hipHostMalloc(void **ptr, size_t size, unsigned int)
{
    const hipError_t e = enter("pin");
    if (e != hipSuccess) return e;
    *ptr = std::malloc(size);
    g_livePinned.insert(*ptr);
    ++g_pinnedAllocated;
    return hipSuccess;
}
hipError_t hipHostFree(void *ptr)
{
    if (!g_livePinned.erase(ptr)) return hipErrorInvalidValue;
    ++g_pinnedFreed;
    std::free(ptr);
    return enter("unpin");
}

} // extern "C"

namespace
{

void test_fence()
{
    const hipStream_t s = stream(1);
    {
        Fence f;
        CHECK(f.wait(s) == PROSPER_PT_OK && f.host_wait() == PROSPER_PT_OK && f.passed());
        CHECK(f.event() == nullptr);
        CHECK(g_log.empty()); // never recorded: nothing was asked of the runtime, no event exists
        CHECK(f.record(s) == PROSPER_PT_OK);
        CHECK(f.event() != nullptr && count("create") == 1 && count("record") == 1);
        CHECK(f.wait(stream(2)) == PROSPER_PT_OK && g_log.back().op == "wait" && g_log.back().stream == stream(2));
        CHECK(f.host_wait() == PROSPER_PT_OK && g_log.back().op == "host_wait");
        CHECK(f.record(s) == PROSPER_PT_OK && count("create") == 1); // the one event again
        g_failOnce = "wait";
        CHECK(f.wait(s) == PROSPER_PT_ERR_HIP && !g_lastError.empty());
    }
    CHECK(count("destroy") == 1 && g_liveEvents.empty());
    {
        Fence f;
        g_failOnce = "record";
        CHECK(f.record(s) == PROSPER_PT_ERR_HIP);
        CHECK(f.event() == nullptr); // a record that failed is no record
        const size_t at = g_log.size();
        CHECK(f.wait(s) == PROSPER_PT_OK && g_log.size() == at);
    }
    CHECK(g_liveEvents.empty());
}

void test_version_ring()
{
    const hipStream_t a = stream(1), b = stream(2);
    {
        // the frame loop: the render's chain writes the next version, behind that version's last readers, and reads it
        VersionRing<3> ring;
        const uint32_t want[7] = {1, 2, 0, 1, 2, 0, 1};
        for (uint32_t i = 0; i < 7; ++i)
        {
            const uint32_t before = ring.cur, v = ring.next();
            CHECK(v == want[i] && ring.cur == before); // next() changes nothing
            size_t at = g_log.size();
            CHECK(ring.wait_free(v, a) == PROSPER_PT_OK);
            // versions 1, 2 and 0 have not been read when they are first written; from then on each has, once
            CHECK(count("wait", at) == (i < 3 ? 0u : 1u) && g_log.size() == at + (i < 3 ? 0u : 1u));
            ring.commit(v);
            CHECK(ring.cur == v);
            at = g_log.size();
            CHECK(ring.mark_read(a) == PROSPER_PT_OK);
            CHECK(count("wait", at) == 0 && count("record", at) == 1); // the same stream as the previous reader: no wait
        }
        // a reader on another stream first waits for the previous readers, then records: one fence stands for all
        size_t at = g_log.size();
        CHECK(ring.mark_read(b) == PROSPER_PT_OK);
        CHECK(g_log.size() == at + 2 && g_log[at].op == "wait" && g_log[at].stream == b && g_log[at + 1].op == "record" &&
              g_log[at + 1].stream == b && g_log[at].event == g_log[at + 1].event);
        at = g_log.size();
        CHECK(ring.mark_read(b) == PROSPER_PT_OK && g_log.size() == at + 1 && g_log[at].op == "record");
        CHECK(ring.mark_read(a) == PROSPER_PT_OK && count("wait", at) == 1);
        // every version's readers (versions 0, 1 and 2 have all been read by now)
        at = g_log.size();
        CHECK(ring.wait_all_free(b) == PROSPER_PT_OK && count("wait", at) == 3 && g_log.size() == at + 3);
        CHECK(count("create") == 3);
    }
    CHECK(g_liveEvents.empty());
    {
        // version 0 belongs to the upload: the ring rotates over 1 .. 3
        VersionRing<4, 1> ring;
        const uint32_t want[7] = {1, 2, 3, 1, 2, 3, 1};
        for (uint32_t i = 0; i < 7; ++i)
        {
            CHECK(ring.next() == want[i]);
            ring.commit(ring.next());
        }
        const size_t at = g_log.size();
        CHECK(ring.wait_all_free(a) == PROSPER_PT_OK && g_log.size() == at); // nothing was ever read
    }
}

void test_staging_ring()
{
    const hipStream_t s = stream(1);
    {
        StagingRing<uint8_t> ring;
        uint8_t *buffers[9] = {};
        const void *copyEvent[9] = {};
        for (uint32_t i = 0; i < 9; ++i)
        {
            const size_t at = g_log.size();
            CHECK(ring.acquire(64, false, &buffers[i]) == PROSPER_PT_OK);
            CHECK(buffers[i] != nullptr && ring.pending_buffer() == buffers[i]);
            buffers[i][63] = (uint8_t)i; // (the whole size is there)
            if (i < kStagingBuffers)
                CHECK(count("host_wait", at) == 0 && count("pin", at) == 1); // a new buffer each: nothing to wait for
            else
            {
                // the buffer of four updates ago, behind ITS copy and no other
                CHECK(buffers[i] == buffers[i - kStagingBuffers] && count("pin", at) == 0);
                CHECK(count("host_wait", at) == 1 && count("host_wait", at, copyEvent[i - kStagingBuffers]) == 1);
            }
            for (uint32_t j = i < kStagingBuffers ? 0 : i - kStagingBuffers + 1; j < i; ++j) CHECK(buffers[j] != buffers[i]);
            CHECK(ring.copy_enqueued(s) == PROSPER_PT_OK);
            CHECK(g_log.back().op == "record" && g_log.back().stream == s);
            copyEvent[i] = g_log.back().event;
        }
        CHECK(count("host_wait") == 5 && g_pinnedAllocated == (int)kStagingBuffers);
    }
    CHECK(g_liveEvents.empty() && g_livePinned.empty());
    {
        // an update nobody consumed is overwritten in place
        StagingRing<uint8_t> ring;
        uint8_t *first = nullptr, *again = nullptr, *other = nullptr;
        CHECK(ring.acquire(16, false, &first) == PROSPER_PT_OK);
        size_t at = g_log.size();
        CHECK(ring.acquire(16, true, &again) == PROSPER_PT_OK && again == first);
        CHECK(g_log.size() == at); // its copy was never enqueued: no wait, no allocation
        // ... one whose copy was enqueued - by a flush that failed later on and left the update pending - behind that copy
        CHECK(ring.copy_enqueued(s) == PROSPER_PT_OK);
        const void *copy = g_log.back().event;
        at = g_log.size();
        CHECK(ring.acquire(16, true, &again) == PROSPER_PT_OK && again == first);
        CHECK(g_log.size() == at + 1 && g_log[at].op == "host_wait" && g_log[at].event == copy);
        at = g_log.size();
        CHECK(ring.acquire(16, true, &again) == PROSPER_PT_OK && again == first && g_log.size() == at); // (waited for already)
        CHECK(ring.copy_enqueued(s) == PROSPER_PT_OK);
        // the ring did not advance meanwhile: the next update takes the second buffer
        at = g_log.size();
        CHECK(ring.acquire(16, false, &other) == PROSPER_PT_OK && other != first && count("pin", at) == 1 && count("host_wait", at) == 0);
        // an acquire that fails hands nothing out and holds nothing
        CHECK(ring.copy_enqueued(s) == PROSPER_PT_OK);
        g_failOnce = "pin";
        uint8_t *none = nullptr;
        CHECK(ring.acquire(16, false, &none) == PROSPER_PT_ERR_HIP && none == nullptr);
    }
    CHECK(g_liveEvents.empty() && g_livePinned.empty());
}

// what flush_pending_lights does with its rings (prosper_amd/csrc/pt_scene_updates.cpp): commit after the last enqueue
struct Resource
{
    VersionRing<3> versions;
    StagingRing<uint8_t> staging;
    Fence ready;
    bool pending = false;
    int stage(uint8_t value)
    {
        uint8_t *p = nullptr;
        if (const int rc = staging.acquire(4, pending, &p)) return rc;
        p[0] = value;
        pending = true;
        return PROSPER_PT_OK;
    }
    int flush(hipStream_t s)
    {
        if (!pending) return PROSPER_PT_OK;
        const uint32_t v = versions.next();
        int rc;
        if ((rc = versions.wait_free(v, s))) return rc;
        if ((rc = staging.copy_enqueued(s))) return rc;
        if ((rc = ready.record(s))) return rc;
        versions.commit(v);
        pending = false;
        return PROSPER_PT_OK;
    }
};

void test_commit_after_success()
{
    const hipStream_t s = stream(1);
    {
        Resource r;
        CHECK(r.stage(1) == PROSPER_PT_OK && r.flush(s) == PROSPER_PT_OK && r.versions.cur == 1 && !r.pending);
        CHECK(r.versions.mark_read(s) == PROSPER_PT_OK);
        const uint8_t *staged = nullptr;
        // what fails: the record behind the staging copy; then the creation of the next staging buffer's fence
        for (const char *failing : {"record", "create"})
        {
            CHECK(r.stage(2) == PROSPER_PT_OK);
            staged = r.staging.pending_buffer();
            const uint32_t before = r.versions.cur;
            g_failOnce = failing;
            CHECK(r.flush(s) == PROSPER_PT_ERR_HIP);
            CHECK(g_failOnce.empty());                      // (the failure was met)
            CHECK(r.versions.cur == before && r.pending);   // the old version stays current, the update stays pending
            CHECK(r.stage(3) == PROSPER_PT_OK && r.staging.pending_buffer() == staged); // ... and is replaced in its buffer
            CHECK(r.flush(s) == PROSPER_PT_OK && r.versions.cur == (before + 1u) % 3u && !r.pending);
            CHECK(r.ready.event() != nullptr);
        }
    }
    CHECK(g_liveEvents.empty() && g_livePinned.empty());
}

void test_stream()
{
    {
        Stream s;
        CHECK(s.get() == nullptr && g_log.empty());
        CHECK(s.create() == PROSPER_PT_OK && s.get() != nullptr && count("stream_create") == 1);
        const hipStream_t made = s.get();
        CHECK(s.create() == PROSPER_PT_OK && s.get() == made && count("stream_create") == 1); // the one stream again
    }
    CHECK(count("stream_destroy") == 1 && g_log.back().stream != nullptr && g_liveStreams.empty());
    size_t at = 0;
    {
        Stream s;
        g_failOnce = "stream_create";
        CHECK(s.create() == PROSPER_PT_ERR_HIP && s.get() == nullptr && !g_lastError.empty());
        at = g_log.size();
    }
    CHECK(g_log.size() == at); // nothing was made: the destructor asked nothing of the runtime
}

void test_launch_timeline()
{
    const hipStream_t a = stream(1), b = stream(2);
    constexpr uint32_t kEvents = kMaxTimedLaunches + 1u;
    static_assert(kMaxTimedLaunches == 96, "the capacity the render's launchers were sized for");
    {
        LaunchTimeline t;
        CHECK(t.create() == PROSPER_PT_OK && count("create_timed") == kEvents && g_log.size() == kEvents);
        std::vector<const void *> events;
        for (const Call &c : g_log) events.push_back(c.event);
        CHECK(t.create() == PROSPER_PT_OK && g_log.size() == kEvents); // a second create makes none
        // mark: event i on the stream of the launch; close: the event behind the last interval
        const uint32_t stages[6] = {0, 1, 2, 1, 2, 3};
        t.begin();
        for (uint32_t i = 0; i < 6; ++i)
        {
            t.mark(stages[i], i == 5 ? b : a);
            CHECK(g_log.back().op == "record" && g_log.back().event == events[i] && g_log.back().stream == (i == 5 ? b : a));
            g_msFrom[events[i]] = 0.25f * (float)(1u << i); // 0.25, 0.5, 1, 2, 4, 8: sums are exact
        }
        t.close(b);
        CHECK(g_log.back().op == "record" && g_log.back().event == events[6] && g_log.back().stream == b);
        CHECK(t.intervals() == 6 && count("record") == 7);
        CHECK(t.wait() == PROSPER_PT_OK && g_log.back().op == "host_wait" && g_log.back().event == events[6]);
        float ms[PROSPER_PT_MAX_KERNELS] = {}, total = 0.0f;
        uint32_t launches[PROSPER_PT_MAX_KERNELS] = {};
        size_t at = g_log.size();
        CHECK(t.add_to(ms, launches, &total) == PROSPER_PT_OK && count("elapsed", at) == 6 && g_log.size() == at + 6);
        for (uint32_t i = 0; i < 6; ++i) CHECK(g_log[at + i].event == events[i] && g_log[at + i].stream == events[i + 1]);
        CHECK(ms[0] == 0.25f && ms[1] == 2.5f && ms[2] == 5.0f && ms[3] == 8.0f && total == 15.75f);
        CHECK(launches[0] == 1 && launches[1] == 2 && launches[2] == 2 && launches[3] == 1);
        for (uint32_t st = 4; st < PROSPER_PT_MAX_KERNELS; ++st) CHECK(ms[st] == 0.0f && launches[st] == 0); // never marked
        // ... INTO the caller's sums: a second timeline (a launch chain's) adds to what is there
        CHECK(t.add_to(ms, launches, &total) == PROSPER_PT_OK && ms[1] == 5.0f && launches[1] == 4 && total == 31.5f);
        g_failOnce = "elapsed";
        CHECK(t.add_to(ms, launches, &total) == PROSPER_PT_ERR_HIP);
        // begin: the next render's intervals start at the first event again
        t.begin();
        CHECK(t.intervals() == 0);
        t.mark(2, a);
        CHECK(g_log.back().event == events[0] && t.intervals() == 1);
        // launches beyond the capacity go untimed, and close still records on the last event
        t.begin();
        at = g_log.size();
        for (uint32_t i = 0; i < kMaxTimedLaunches; ++i) t.mark(1, a);
        CHECK(count("record", at) == kMaxTimedLaunches && g_log.back().event == events[kMaxTimedLaunches - 1u]);
        at = g_log.size();
        t.mark(1, a); // the 97th
        CHECK(g_log.size() == at && t.intervals() == kMaxTimedLaunches);
        t.close(a);
        CHECK(g_log.size() == at + 1 && g_log.back().op == "record" && g_log.back().event == events[kMaxTimedLaunches]);
        CHECK(t.wait() == PROSPER_PT_OK && g_log.back().event == events[kMaxTimedLaunches]);
        std::fill(ms, ms + PROSPER_PT_MAX_KERNELS, 0.0f);
        std::fill(launches, launches + PROSPER_PT_MAX_KERNELS, 0u);
        CHECK(t.add_to(ms, launches, &total) == PROSPER_PT_OK && launches[1] == kMaxTimedLaunches && launches[0] == 0);
    }
    CHECK(count("destroy") == kEvents && g_liveEvents.empty());
    g_msFrom.clear();
    for (const uint32_t k : {1u, 40u, kEvents})
    {
        // a create that fails at the k-th event: the destructor gives back the k - 1 that were made
        g_log.clear();
        {
            LaunchTimeline t;
            g_failAt = k;
            CHECK(t.create() == PROSPER_PT_ERR_HIP && !g_lastError.empty());
            CHECK(g_failAt == 0 && count("create_timed") == k - 1u && count("create_timed!") == 1);
        }
        CHECK(count("destroy") == k - 1u && g_liveEvents.empty());
    }
    {
        // ... and a create after the failure makes only what is missing
        g_log.clear();
        LaunchTimeline t;
        g_failAt = 40;
        CHECK(t.create() == PROSPER_PT_ERR_HIP && t.create() == PROSPER_PT_OK && count("create_timed") == kEvents);
    }
    CHECK(g_liveEvents.empty());
    {
        // the passes' timed events share the creation: N + 1 events, one interval per stage
        g_log.clear();
        StageEvents<2> e;
        CHECK(!e.created() && e.create() == PROSPER_PT_OK && e.created() && count("create_timed") == 3);
        g_msFrom[e.events[0]] = 1.5f;
        g_msFrom[e.events[1]] = 0.5f;
        float ms[2] = {};
        CHECK(e.elapsed(ms) == PROSPER_PT_OK && ms[0] == 1.5f && ms[1] == 0.5f && count("host_wait", 0, e.events[2]) == 1);
    }
    g_msFrom.clear();
    CHECK(g_liveEvents.empty());
}

} // namespace

int main()
{
    void (*const tests[])() = {test_fence, test_version_ring, test_staging_ring, test_commit_after_success, test_stream,
                               test_launch_timeline};
    for (auto test : tests)
    {
        g_log.clear();
        g_pinnedAllocated = g_pinnedFreed = 0;
        test();
    }
    // every owner is gone: each event, pinned buffer and stream was given back exactly once (a second time fails in the fake)
    CHECK(g_eventsCreated > 0 && g_eventsCreated == g_eventsDestroyed && g_liveEvents.empty() && g_livePinned.empty());
    CHECK(g_streamsCreated > 0 && g_streamsCreated == g_streamsDestroyed && g_liveStreams.empty());
    if (g_failures) std::fprintf(stderr, "%d check(s) failed\n", g_failures);
    else std::printf("sync rings ok: %d events\n", g_eventsCreated);
    return g_failures ? 1 : 0;
}
