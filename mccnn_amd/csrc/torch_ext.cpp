// torch_ext.cpp -- the PyTorch-ROCm side of the native step executor: autograd node, device buffers and streams for
// mccnn_geometry_* / mccnn_conv_* (include/mccnn.h), so that a convolution costs the host ONE Python -> C++ call in the
// forward pass and NONE in the backward pass (the autograd engine calls the C++ node directly).
//
// torch only supplies what the C-ABI leaves to its caller: device memory (at::empty -- the library never allocates), the
// current HIP stream and the autograd graph. Every kernel launch goes through libmccnn_hip.so. Built by
// mccnn_amd/build.py with g++ against the torch headers (host code only, no kernels here); mccnn_amd/native.py falls
// back to the ctypes form of the same calls when this module is not built.
#include <torch/extension.h>
#include <execinfo.h>
#include <torch/csrc/autograd/function.h>
#include <torch/csrc/autograd/functions/utils.h>
#include <torch/csrc/autograd/saved_variable.h>
#include <c10/hip/HIPStream.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <hip/hip_runtime_api.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <deque>
#include <functional>
#include <map>
#include <thread>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "mccnn.h"
#include "debug_opts.h"
#include "bn_drop.h"

namespace {

using at::Tensor;

struct CapacityError : std::runtime_error {
    int edges;
    CapacityError(int e) : std::runtime_error("neighbour list longer than the geometry's capacity"), edges(e) {}
};

void check(int rc, const char* what) {
    if (rc == 0) return;
    throw std::runtime_error(std::string(what) + " failed: " + mccnn_error_string(rc) + " (code " + std::to_string(rc) + ")");
}

// The HIP runtime's current device for the length of a call: the library launches on streams of its tensors' device and
// that device has to be current on the launching thread (a caller working with several devices may have another one set).
struct DevGuard {
    int prev = 0;
    bool changed = false;
    explicit DevGuard(int d) {
        if (hipGetDevice(&prev) == hipSuccess && d != prev && d >= 0) changed = hipSetDevice(d) == hipSuccess;
    }
    ~DevGuard() {
        if (changed) (void)hipSetDevice(prev);
    }
    DevGuard(const DevGuard&) = delete;
    DevGuard& operator=(const DevGuard&) = delete;
};

void* cur_stream(const Tensor& t) { return (void*)c10::hip::getCurrentHIPStream(t.device().index()).stream(); }
// a raw stream as PyTorch's allocator knows it (pool selection: HIPStreamGuard; consumers: Tensor::record_stream)
c10::Stream as_torch_stream(void* s, int dev) {
    return c10::hip::getStreamFromExternalMasqueradingAsCUDA((hipStream_t)s, (c10::DeviceIndex)dev).unwrap();
}

hipEvent_t take_event_fwd();
void give_event_fwd(hipEvent_t e);

// grow-only scratch per (thread, device, stream): consecutive calls on a stream are stream-ordered and may share it
Tensor& scratch(size_t bytes, const Tensor& like, void* stream) {
    thread_local std::map<std::pair<int, void*>, Tensor> pool;
    Tensor& t = pool[{(int)like.device().index(), stream}];
    if (bytes < 256) bytes = 256;
    if (!t.defined() || (size_t)t.numel() < bytes) {
        // the old block goes back to the allocator of the CALLING thread's current stream, which need not be `stream`:
        // what `stream` still runs on it has to be over first (rare: the scratch only grows)
        if (t.defined()) (void)hipStreamSynchronize((hipStream_t)stream);
        t = at::empty({(int64_t)(bytes + bytes / 4)}, like.options().dtype(at::kByte));
        // ... and the NEW block comes from the caching allocator's pool of the calling thread's current stream: the
        // allocator hands out a block its last owner freed a moment ago, because work enqueued on THAT stream is ordered
        // behind the old owner's. Work on `stream` is not -- a helper thread's scratch used to be written on its side
        // stream while convolution kernels still read the block as THEIR scratch (wrong level sizes of a prefetched
        // hierarchy, wrong outputs: tools/soak_network.py SOAK_CFG=cfg4 SOAK_DEEP=1). `stream` first waits for what
        // the allocation stream holds now.
        void* alloc = cur_stream(like);
        if (alloc != stream) {
            hipEvent_t ev = take_event_fwd();
            if (hipEventRecord(ev, (hipStream_t)alloc) == hipSuccess) (void)hipStreamWaitEvent((hipStream_t)stream, ev, 0);
            give_event_fwd(ev);
        }
    }
    return t;
}

// pinned words the count pass stores the edge total into (device-accessible host memory: no copy is enqueued)
std::mutex g_slot_mutex;
std::vector<Tensor> g_slots;
void poll_parked();
Tensor take_slot() {
    poll_parked();
    {
        std::lock_guard<std::mutex> lk(g_slot_mutex);
        if (!g_slots.empty()) {
            Tensor t = g_slots.back();
            g_slots.pop_back();
            return t;
        }
    }
    return at::empty({1}, at::TensorOptions().dtype(at::kInt).pinned_memory(true));
}
void give_slot(Tensor t) {
    std::lock_guard<std::mutex> lk(g_slot_mutex);
    if (g_slots.size() < 256) g_slots.push_back(std::move(t));
}
// A geometry destroyed before its edge total arrived (dropped right after being queued, or on an exception path): the count
// pass may still WRITE the word, so the slot is neither reused nor returned to the host allocator until the build has
// retired -- parked with an event recorded behind the build, polled whenever a slot is taken.
hipEvent_t take_event();
void give_event(hipEvent_t e);
struct ParkedSlot { Tensor slot; hipEvent_t ev; };
std::vector<ParkedSlot> g_parked;   // (under g_slot_mutex)
void park_slot(Tensor t, hipEvent_t ev) {
    std::lock_guard<std::mutex> lk(g_slot_mutex);
    g_parked.push_back({std::move(t), ev});
}
void poll_parked() {
    std::vector<hipEvent_t> done;
    {
        std::lock_guard<std::mutex> lk(g_slot_mutex);
        for (size_t k = 0; k < g_parked.size();) {
            ParkedSlot& p = g_parked[k];
            const bool arrived = *reinterpret_cast<volatile int*>(p.slot.data_ptr()) >= 0;
            if (arrived || !p.ev || hipEventQuery(p.ev) == hipSuccess) {
                if (p.ev) done.push_back(p.ev);
                if (g_slots.size() < 256) g_slots.push_back(std::move(p.slot));
                g_parked[k] = std::move(g_parked.back());
                g_parked.pop_back();
            } else {
                ++k;
            }
        }
    }
    for (hipEvent_t e : done) give_event(e);
}

// Side streams for geometry builds issued ahead of their first use (ConvolutionBuilder's learned prefetch): the chains of
// a step's geometries are independent of each other and of the features, so they run side by side -- each is a dozen
// small dependent kernels that leave the chip nearly empty -- and the layer that consumes one waits for its event.
constexpr int kSideStreams = 4;
constexpr int kMaxDevices = 16;
int device_now() {
    int d = 0;
    (void)hipGetDevice(&d);
    return (d >= 0 && d < kMaxDevices) ? d : 0;
}
// (streams of the CURRENT device: every entry point below runs under a guard of its tensors' device)
hipStream_t side_stream(int k) {
    static hipStream_t streams[kMaxDevices][kSideStreams] = {};
    static bool made[kMaxDevices] = {};
    static std::mutex m;
    const int d = device_now();
    std::lock_guard<std::mutex> lk(m);
    if (!made[d]) {
        for (int i = 0; i < kSideStreams; ++i)
            if (hipStreamCreateWithFlags(&streams[d][i], hipStreamNonBlocking) != hipSuccess) streams[d][i] = nullptr;
        made[d] = true;
    }
    return streams[d][((k % kSideStreams) + kSideStreams) % kSideStreams];
}
void hip_check(hipError_t e, const char* what) {
    if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}

// events are pooled: creating and destroying one per geometry cost more than the record and the wait together
std::mutex g_event_mutex;
std::vector<hipEvent_t> g_events;
hipEvent_t take_event() {
    {
        std::lock_guard<std::mutex> lk(g_event_mutex);
        if (!g_events.empty()) {
            hipEvent_t e = g_events.back();
            g_events.pop_back();
            return e;
        }
    }
    hipEvent_t e = nullptr;
    hip_check(hipEventCreateWithFlags(&e, hipEventDisableTiming), "hipEventCreate");
    return e;
}
void give_event(hipEvent_t e) {
    std::lock_guard<std::mutex> lk(g_event_mutex);
    if (g_events.size() < 256) g_events.push_back(e);
    else (void)hipEventDestroy(e);
}
hipEvent_t take_event_fwd() { return take_event(); }
void give_event_fwd(hipEvent_t e) { give_event(e); }

// A helper thread starts with device 0 current; every job names the device of its tensors first (one process per GPU sets
// its device on the calling thread only -- kernel launches, memsets and event records of a job go to streams of THAT
// device and need it current on the issuing thread as well).
void enter_device(int dev) {
    thread_local int current = -1;
    if (dev != current && hipSetDevice(dev) == hipSuccess) current = dev;
}

// The launches of a side-stream build are ISSUED by a helper thread: a step's geometries are a dozen launches each
// (~35 us of host time), and the calling thread has the layers to issue. One thread, jobs in order (a geometry that
// shares another one's grid is queued behind it). MCCNN_ISSUE_THREAD=0: the calling thread issues them itself.
thread_local bool t_helper_thread = false;

class Issuer {
public:
    // 0: geometry builds of the step in flight; 1: point hierarchies of the NEXT batch (those jobs block on read-backs);
    // 2: row plans / transposed lists of the step's geometries (those jobs wait for edge totals)
    static Issuer& get(int which = 0) {
        static Issuer inst[3];
        return inst[which];
    }
    static bool enabled() {
        static const bool on = mccnn::debug_int("issue_thread", 1) != 0;
        return on;
    }
    void push(std::function<void()> job) {
        bool queued = false;
        {
            std::lock_guard<std::mutex> lk(m_);
            if (!stop_) {   // (retired: the job runs on the caller's thread)
                if (!started_) {
                    th_ = std::thread([this] { run(); });
                    started_ = true;
                }
                q_.push_back(std::move(job));
                queued = true;
            }
        }
        if (queued) cv_.notify_one();
        else job();
    }
    // Runs the queued jobs to the end and joins the thread; later jobs run on the caller's thread. Called from Python's
    // atexit (shutdown_helpers): a job -- or its destruction -- may drop the last reference to a tensor that has a Python
    // object, which takes the GIL; on a helper thread during interpreter finalisation that attempt ends the thread with a
    // forced unwind (std::terminate). After this no helper thread exists that could hold such a reference.
    void retire() {
        {
            std::lock_guard<std::mutex> lk(m_);
            stop_ = true;
        }
        cv_.notify_all();
        if (started_ && th_.joinable()) th_.join();
    }
    ~Issuer() { retire(); }

private:
    void run() {
        t_helper_thread = true;
        mccnn_debug_wait_accounting(0);
        for (;;) {
            std::function<void()> job;
            {
                std::unique_lock<std::mutex> lk(m_);
                cv_.wait(lk, [this] { return stop_ || !q_.empty(); });
                if (q_.empty()) return;
                job = std::move(q_.front());
                q_.pop_front();
            }
            static const int delay_us = mccnn::debug_int("job_delay_us", 0);
            if (delay_us > 0) {   // fault injection of the soak tests: a random pause of 0 .. delay_us before every job
                static thread_local unsigned lcg = 12345u + (unsigned)(uintptr_t)this;
                lcg = lcg * 1664525u + 1013904223u;
                std::this_thread::sleep_for(std::chrono::microseconds((lcg >> 8) % (unsigned)(delay_us + 1)));
            }
            job();
        }
    }
    std::mutex m_;
    std::condition_variable cv_;
    std::deque<std::function<void()>> q_;
    std::thread th_;
    bool started_ = false, stop_ = false;
};

void count_wait(std::chrono::steady_clock::time_point t0);

// how often a geometry nobody joined ordered its CALLER's stream behind its kernels when it died (debug_counters(): the
// regression check of NOTES round-6 item 6c -- zero would mean the waits are being skipped again)
std::atomic<long long> g_caller_orderings{0};

// The per-point density of ONE (grid, window) -- pdfMode='point': density [n,1] f32 and counts [n,1] i32 of the grid's sorted
// points. The grid's owner keeps one per window (mccnn_amd.native: Geometry.point_density) and every geometry over that grid
// and window holds it: the first build computes it, later ones only expand it over their lists. `ev` is recorded behind the
// build that wrote it; a sharer on another stream waits for it (the join of a grid_from sharer behind its owner's grid, for
// the density). The tensors come from the pool of the writer's buffers (`alloc_stream`); every other stream that reads them
// is made known to the allocator (record_stream), like the grid arrays of a geometry that has a pool of its own.
struct PointPdf {
    Tensor density, counts;
    void* alloc_stream = nullptr;
    void* write_stream = nullptr;       // the stream the sweep runs on
    hipEvent_t ev = nullptr;
    std::atomic<int> recorded{0};       // 0 while the helper thread has not issued the writer's build yet
    void wait_recorded() {
        int spins = 0;
        while (!recorded.load(std::memory_order_acquire))
            if (++spins > 2000) std::this_thread::yield();
    }
    void mark(void* stream) {            // behind the writer's build, on its stream
        if (ev && hipEventRecord(ev, (hipStream_t)stream) != hipSuccess) { give_event_fwd(ev); ev = nullptr; }
        recorded.store(1, std::memory_order_release);
    }
    // `stream` reads (or expands) the density: ordered behind the sweep, and known to the allocator
    void order(void* stream) {
        if (stream == write_stream && stream == alloc_stream) return;
        if (stream != write_stream) {
            wait_recorded();
            if (ev && hipStreamWaitEvent((hipStream_t)stream, ev, 0) != hipSuccess) throw std::runtime_error("point density: hipStreamWaitEvent");
        }
        if (stream != alloc_stream) {
            const c10::Stream reader = as_torch_stream(stream, (int)density.device().index());
            density.record_stream(reader);
            counts.record_stream(reader);
        }
    }
    ~PointPdf() { if (ev) give_event_fwd(ev); }
};

struct Geo {
    mccnn_geometry_t* h = nullptr;
    std::shared_ptr<PointPdf> pp;   // the per-point density its PDFs are expanded from (null: edge mode)
    std::atomic<int> issued{1};    // 0 while the helper thread has not issued this geometry's build yet
    int build_rc = 0;
    hipEvent_t event = nullptr;    // recorded behind a build on a side stream; its consumers wait for it once
    bool needs_wait = false;
    int side = -1;                 // index of the side stream the build ran on (-1: the caller's stream)
    void* alloc_stream = nullptr;  // the stream the buffers were allocated on (the caller's at build time)
    // own_pool: `buf` and the prebuilt pieces come from the caching allocator's pool of the build's OWN side stream (a
    // block it hands out was last used on that stream: the build needs no ordering behind the calling stream for its
    // memory) and the build waits for the event of the prefetched hierarchy it reads instead of for everything the
    // calling stream holds -- the next batch's geometry then starts when it is asked for, not when the device has
    // finished the step in flight. Every stream that joins the build is made known to the allocator (record_stream).
    bool own_pool = false;
    void* caller_stream = nullptr;  // own_pool: the stream of the thread that asked for the build (where its inputs are consumed)
    // (... which is a NULL handle when that thread runs on the device's default stream -- the usual case: `has_caller`, not the
    // handle, says whether it is set. Round 6: the waits below were skipped for exactly that stream, and a loop that prefetched
    // geometry it never consumed let the next hierarchy overwrite level tensors that builds / plan kernels were still reading.)
    bool has_caller = false;
    void order_caller_behind(hipEvent_t ev) {
        if (!(own_pool && has_caller && caller_waits())) return;
        g_caller_orderings.fetch_add(1, std::memory_order_relaxed);
        (void)hipStreamWaitEvent((hipStream_t)caller_stream, ev, 0);
    }
    static bool caller_waits() { static const bool on = mccnn::debug_int("caller_join_off", 0) == 0; return on; }   // (fault injection: the round-6 bug back)
    Tensor buf, slot;
    std::vector<Tensor> keep, attached;
    std::shared_ptr<Geo> grid_owner;
    int n = 0, m = 0, nc = 0, B = 0;
    int64_t e_cap = 0;
    std::atomic<int> e{-1};   // (also set by the helper thread that reads the total for the pieces it issues)
    int uses = 0;  // layers convolved over this geometry so far (the builder counts)
    std::atomic<int> pieces_issued{1};  // 0 while the helper thread still has pieces of this geometry to attach / issue
    void wait_build_issued_nothrow() {
        int spins = 0;
        while (!issued.load(std::memory_order_acquire))
            if (++spins > 2000) std::this_thread::yield();
    }
    void wait_issued_nothrow() {
        if (issued.load(std::memory_order_acquire) && pieces_issued.load(std::memory_order_acquire)) return;
        // (time spent here is a WAIT for a helper thread, which in turn waits for the device: counted with the waits for
        // device-side sizes, not with the calling thread's own work -- wait_ns())
        const auto t0 = std::chrono::steady_clock::now();
        wait_build_issued_nothrow();
        int spins = 0;
        while (!pieces_issued.load(std::memory_order_acquire))
            if (++spins > 2000) std::this_thread::yield();
        count_wait(t0);
    }
    // the build's launches (and its event record) have been issued, and so have the pieces asked for with it: nothing
    // of the handle is touched before
    void wait_issued() {
        wait_issued_nothrow();
        if (build_rc) {
            const int rc = build_rc;
            build_rc = 0;
            check(rc, "geometry_build");
        }
    }
    // order `stream` behind the side-stream build (once: every later use of the geometry is on that stream as well)
    // Pieces prebuilt on the side stream come in two stages with an event each: the forward row plan (and the records),
    // then the transposed list and the transposed row plan. A forward pass waits for the first only -- unless it would
    // have to build something itself (no forward plan among the pieces, another `avg`), which must not overlap the
    // second stage: both write the shared records. A backward pass waits for both.
    void join(void* stream, bool everything = true) {
        wait_issued();
        bool joined = false;
        if (needs_wait && event) {
            hip_check(hipStreamWaitEvent((hipStream_t)stream, event, 0), "hipStreamWaitEvent");
            needs_wait = false;
            joined = true;
        }
        if (plan_wait && plan_event) {
            hip_check(hipStreamWaitEvent((hipStream_t)stream, plan_event, 0), "hipStreamWaitEvent");
            plan_wait = false;
            joined = true;
        }
        if (tr_wait && tr_event && (everything || !(have & 1))) {
            hip_check(hipStreamWaitEvent((hipStream_t)stream, tr_event, 0), "hipStreamWaitEvent");
            tr_wait = false;
            joined = true;
        }
        if (joined && own_pool && stream != alloc_stream && buf.defined()) {
            const c10::Stream consumer = as_torch_stream(stream, (int)buf.device().index());
            buf.record_stream(consumer);
            for (Tensor& t : attached) t.record_stream(consumer);
            // (the inputs the library borrowed pointers of: a consumer on a stream other than the one that made the geometry
            // reads through them too -- the grid's sorted copies are ours, the centres are the caller's)
            if (stream != caller_stream)
                for (Tensor& t : keep) if (t.defined()) t.record_stream(consumer);
        }
    }
    ~Geo() {
        wait_issued_nothrow();
        const bool total_pending = slot.defined() && e.load(std::memory_order_relaxed) < 0 &&
                                   *reinterpret_cast<volatile int*>(slot.data_ptr()) < 0;
        hipEvent_t slot_ev = nullptr;
        // a grid shared from a geometry on ANOTHER side stream's pool: its memory may go back to that pool right after this
        // (the owner outlives its users), and this build's reads of it are ordered on this stream only
        if (event && build_rc == 0 && side >= 0 && grid_owner && grid_owner->own_pool && grid_owner->side != side)
            (void)hipStreamWaitEvent((hipStream_t)grid_owner->alloc_stream, event, 0);
        if (event) {
            // never consumed: the buffers go back to the allocator of the stream they were taken on -- order that
            // stream behind the build first, or the next owner of the memory could race with it
            // (this destructor may run on the helper thread: the allocation stream is the one remembered at build time)
            if (needs_wait && buf.defined() && build_rc == 0) {
                (void)hipStreamWaitEvent((hipStream_t)alloc_stream, event, 0);
                // own pool: the INPUTS (`keep`: tensors of the hierarchy, freed after this) are known to the allocator as
                // used on the caller's stream only -- a build nobody joined has to be over before that stream moves on
                order_caller_behind(event);
            }
            if (total_pending && build_rc == 0) slot_ev = event;   // (the event of the build: the parked slot keeps it)
            else give_event(event);
        } else if (total_pending && build_rc == 0 && buf.defined()) {
            // built on the caller's stream: an event recorded there now lies behind the count pass
            try {
                slot_ev = take_event();
                if (hipEventRecord(slot_ev, (hipStream_t)alloc_stream) != hipSuccess) { give_event(slot_ev); slot_ev = nullptr; }
            } catch (const std::exception&) {
                slot_ev = nullptr;
            }
        }
        if (plan_event) {
            if (plan_wait && buf.defined()) {
                (void)hipStreamWaitEvent((hipStream_t)alloc_stream, plan_event, 0);
                order_caller_behind(plan_event);
            }
            give_event(plan_event);
        }
        if (tr_event) {
            if (tr_wait && buf.defined()) {
                (void)hipStreamWaitEvent((hipStream_t)alloc_stream, tr_event, 0);
                order_caller_behind(tr_event);
            }
            give_event(tr_event);
        }
        if (h) mccnn_geometry_destroy(h);
        if (slot.defined()) {
            if (!total_pending) give_slot(std::move(slot));
            else if (slot_ev) park_slot(std::move(slot), slot_ev);   // the count pass may still write the word
            else if (build_rc != 0) give_slot(std::move(slot));     // the build never ran: nobody writes it
            else park_slot(std::move(slot), nullptr);                // (no event to be had: recycled on the next poll)
        }
    }
    hipEvent_t plan_event = nullptr;   // recorded behind the forward row plan prebuilt on a side stream (prebuild)
    bool plan_wait = false;
    hipEvent_t tr_event = nullptr;     // ... behind the transposed list / transposed row plan
    bool tr_wait = false;
    int pre_avg = -1;                  // the `avg` the prebuilt plans were made for
    int have = 0;                      // pieces attached so far (mask)
    int plan_side = -1;                // batch builds: the side stream this geometry's row plans / transposed list go to (spread over all of them)

    // The attached pieces of `what` (1 | 2 | 4) on stream ss, forward stage first; one event per stage.
    int issue_pieces(int what, bool avg, hipStream_t ss, void* ws, size_t wsb) {
        int rc = 0;
        if (what & 1) {
            rc = mccnn_geometry_prebuild(h, 1, avg ? 1 : 0, ws, wsb, (void*)ss);
            if (!rc) {
                if (!plan_event) plan_event = take_event();
                if (hipEventRecord(plan_event, ss) != hipSuccess) rc = (int)hipErrorUnknown;
                plan_wait = true;
            }
        }
        if (!rc && (what & 6)) {
            rc = mccnn_geometry_prebuild(h, what & 6, avg ? 1 : 0, ws, wsb, (void*)ss);
            if (!rc) {
                if (!tr_event) tr_event = take_event();
                if (hipEventRecord(tr_event, ss) != hipSuccess) rc = (int)hipErrorUnknown;
                tr_wait = true;
            }
        }
        pre_avg = avg ? 1 : 0;
        return rc;
    }

    // Builds the pieces of `what` (1 forward row plan, 2 transposed row plan, 4 transposed list; the per-edge records
    // come with a plan) on side stream `side_k`, behind this geometry's own build and behind whatever the calling stream
    // holds now (`like`'s stream: the buffers are allocated there). Waits for the edge total. The layers that use the
    // geometry order their stream behind the pieces' event.
    void prebuild(int what, bool avg, int side_k, const Tensor& like) {
        const DevGuard device_guard((int)like.device().index());
        wait_issued();
        const int E = edges(-1);
        if (E <= 0 || E > e_cap) return;   // (an overflowing list is rebuilt by the first layer: nothing to build ahead)
        if (what & 3) what |= 8;           // a plan permutes the per-edge records
        if (what & 2) what |= 4;           // the transposed plan is laid out over the transposed list
        what &= ~have;
        if (!what) return;
        void* main_stream = cur_stream(like);
        hipStream_t ss = side >= 0 ? side_stream(side) : side_stream(side_k);   // behind the build: its own side stream
        if (!ss) return;
        size_t wsb = 256;
        for (int bit = 1; bit <= 8; bit <<= 1) {
            if (!(what & bit)) continue;
            long long bytes = 0, w = 0;
            check(mccnn_geometry_piece_bytes(h, bit, &bytes, &w), "geometry_piece_bytes");
            Tensor t;
            if (own_pool) {   // (with the geometry's buffer: one pool, one stream to order the memory on)
                const c10::hip::HIPStreamGuardMasqueradingAsCUDA own(as_torch_stream((void*)ss, (int)like.device().index()));
                t = at::empty({(int64_t)(bytes > 256 ? bytes : 256)}, like.options().dtype(at::kByte));
            } else {
                t = at::empty({(int64_t)(bytes > 256 ? bytes : 256)}, like.options().dtype(at::kByte));
            }
            check(mccnn_geometry_attach(h, bit, t.data_ptr(), (size_t)t.numel()), "geometry_attach");
            attached.push_back(std::move(t));
            have |= bit;
            if ((size_t)w > wsb) wsb = (size_t)w;
        }
        Tensor& ws = scratch(wsb, like, (void*)ss);
        // the side stream starts behind the calling stream (the memory just allocated may have had readers there) and,
        // being the build's own stream, behind the geometry itself
        if (!own_pool) {
            static thread_local hipEvent_t fork_ev = nullptr;
            if (!fork_ev) hip_check(hipEventCreateWithFlags(&fork_ev, hipEventDisableTiming), "hipEventCreate");
            hip_check(hipEventRecord(fork_ev, (hipStream_t)main_stream), "hipEventRecord");
            hip_check(hipStreamWaitEvent(ss, fork_ev, 0), "hipStreamWaitEvent");
        }
        if (event && side < 0) hip_check(hipStreamWaitEvent(ss, event, 0), "hipStreamWaitEvent");
        check(issue_pieces(what & 7, avg, ss, ws.data_ptr(), (size_t)ws.numel()), "geometry_prebuild");
    }

    int edges(int wait_us) {
        wait_issued();
        if (e < 0 && h) {
            const int v = mccnn_geometry_edges(h, wait_us);
            if (v >= 0) e = v;
        }
        return e;
    }
    std::vector<int64_t> info() {
        wait_issued();
        long long out[16];
        check(mccnn_geometry_info(h, out), "geometry_info");
        return std::vector<int64_t>(out, out + 16);
    }
    // device address of the word that holds the cap a budgeted search chose (0: the geometry has no budget)
    int64_t cap_addr() {
        wait_issued();
        return (int64_t)(uintptr_t)mccnn_geometry_cap(h);
    }
};

void check_dev(const Tensor& t, at::ScalarType dt, const char* name) {
    TORCH_CHECK(t.defined() && t.is_cuda() && t.scalar_type() == dt && t.is_contiguous(), name,
                ": expected a contiguous device tensor of the op's type");
}

struct HierFuture;
// the event recorded behind an ADOPTED prefetched hierarchy (nullptr: not adopted, failed, none)
hipEvent_t hierarchy_ready_event(const std::shared_ptr<HierFuture>& f);
// whether `t` lives in the memory of that hierarchy (its input points / batch ids, boxes, level rows)
bool hierarchy_owns(const std::shared_ptr<HierFuture>& f, const Tensor& t);

// ---- geometries of a step issued as ONE batch (mccnn_geometry_build_batch: one launch per kernel kind over all of them).
// Between begin_geometry_batch() and end_geometry_batch() every build_geometry() call that would go to a side stream is
// only RECORDED (its buffers allocated, its Geo returned); end_geometry_batch() hands the whole list to the helper thread,
// which issues them on ONE side stream and records every geometry's event behind the batch.
struct BatchEntry {
    std::shared_ptr<Geo> g, grid_from;
    mccnn_geometry_request req;
    mccnn_neighbor_cap cap;   // of the request's search (max_neighbors 0: none)
    mccnn_point_pdf point;    // its per-point density (density null: edge mode)
    mccnn_neighbor_budget budget{0};   // its edge budget (0: none)
    bool writes_point = false;   // this request computes the density: its event is recorded behind the batch
};
struct PieceEntry {   // row plans / transposed list of a batched geometry whose list is small: built as a batch as well
    std::shared_ptr<Geo> g;
    int what;
    bool avg;
    char* base;
    long long off[4], len[4];
};
struct GeoBatch {
    bool active = false;
    int side = -1;
    bool background = false;
    std::vector<BatchEntry> entries;
    std::vector<PieceEntry> pieces;
    // The buffers of a batch's geometries ([0]) and of their pieces ([1]) are views of ONE allocation each, sized by what the
    // last batch took: a block that carries record_stream() costs its consumer's QUEUE an event record when it is freed
    // (~3-5 us of queue time), and a step's geometries are all joined by the layers' stream and all die in one reset() --
    // 28 blocks per step of BASELINE cfg4 were 0.14 ms of the queue that bounds the step; two blocks are two records.
    Tensor arena[2];
    int64_t arena_off[2] = {0, 0}, taken[2] = {0, 0};
};
thread_local GeoBatch t_geo_batch;
thread_local int64_t t_arena_want[2] = {0, 0};   // bytes the last batch of this thread took from each arena (0: none yet)
// `bytes` of the batch's arena `k` (allocated on first use under the caller's stream guard), or an undefined tensor: the
// caller then allocates a block of its own (first batch, a batch larger than the last one, batches switched off)
Tensor arena_take(int k, int64_t bytes, const Tensor& like) {
    GeoBatch& b = t_geo_batch;
    const int64_t need = (bytes + 255) / 256 * 256;
    b.taken[k] += need;
    if (!b.active || t_arena_want[k] <= 0) return Tensor();
    if (!b.arena[k].defined()) {
        b.arena[k] = at::empty({t_arena_want[k] + t_arena_want[k] / 16 + 4096}, like.options().dtype(at::kByte));
        b.arena_off[k] = 0;
    }
    if (b.arena_off[k] + need > b.arena[k].numel()) return Tensor();
    Tensor t = b.arena[k].narrow(0, b.arena_off[k], bytes);
    b.arena_off[k] += need;
    return t;
}
void begin_geometry_batch() {
    t_geo_batch.active = Issuer::enabled();
    t_geo_batch.side = -1;
    t_geo_batch.entries.clear();
    t_geo_batch.pieces.clear();
    for (int k = 0; k < 2; ++k) { t_geo_batch.arena[k] = Tensor(); t_geo_batch.arena_off[k] = t_geo_batch.taken[k] = 0; }
}
void end_geometry_batch() {
    GeoBatch& b = t_geo_batch;
    b.active = false;
    for (int k = 0; k < 2; ++k) {   // (the views keep the arenas alive; the next batch is sized by this one)
        if (b.taken[k] > 0) t_arena_want[k] = b.taken[k];
        b.arena[k] = Tensor();
    }
    if (b.entries.empty()) return;
    auto entries = std::make_shared<std::vector<BatchEntry>>(std::move(b.entries));
    b.entries.clear();
    hipStream_t stream = side_stream(b.side);
    const bool background = b.background;
    const int dev = (int)(*entries)[0].g->buf.device().index();
    Issuer::get().push([entries, stream, background, dev] {
        enter_device(dev);
        std::vector<mccnn_geometry_request> reqs;
        std::vector<mccnn_neighbor_cap> caps;
        std::vector<mccnn_point_pdf> points;
        std::vector<mccnn_neighbor_budget> budgets;
        bool any_cap = false, any_point = false, any_budget = false;
        budgets.reserve(entries->size());
        reqs.reserve(entries->size());
        caps.reserve(entries->size());
        points.reserve(entries->size());
        for (BatchEntry& e : *entries) {
            // a grid owner outside this batch has to be issued; one inside it is set up by the same library call
            bool inside = false;
            if (e.grid_from)
                for (BatchEntry& o : *entries) inside = inside || (o.g.get() == e.grid_from.get());
            if (e.grid_from && !inside) e.grid_from->wait_issued_nothrow();
            reqs.push_back(e.req);
            caps.push_back(e.cap);
            any_cap = any_cap || e.cap.max_neighbors > 0 || e.budget.max_edges > 0;   // (a budgeted request may carry a seed)
            budgets.push_back(e.budget);
            any_budget = any_budget || e.budget.max_edges > 0;
            points.push_back(e.point);
            any_point = any_point || e.point.density != nullptr;
        }
        const int prev = background ? mccnn_background_launches(1) : 0;
        int rc = any_budget ? mccnn_geometry_build_batch_budget(reqs.data(), caps.data(), any_point ? points.data() : nullptr, budgets.data(), (int)reqs.size(), (void*)stream)
               : any_point ? mccnn_geometry_build_batch_point(reqs.data(), any_cap ? caps.data() : nullptr, points.data(), (int)reqs.size(), (void*)stream)
                           : mccnn_geometry_build_batch_capped(reqs.data(), any_cap ? caps.data() : nullptr, (int)reqs.size(), (void*)stream);
        if (background) mccnn_background_launches(prev);
        for (BatchEntry& e : *entries) {
            if (e.writes_point) e.g->pp->mark((void*)stream);
            int r = rc;
            if (r == 0 && hipEventRecord(e.g->event, stream) != hipSuccess) r = (int)hipErrorUnknown;
            e.g->build_rc = r;
            e.g->issued.store(1, std::memory_order_release);
        }
    });
    if (b.pieces.empty()) return;
    // ... and the pieces of the small lists among them: ONE job, one launch per kernel kind (mccnn_geometry_prebuild_batch)
    auto pieces = std::make_shared<std::vector<PieceEntry>>(std::move(b.pieces));
    b.pieces.clear();
    const int pside = (*pieces)[0].g->plan_side;
    Issuer::get(2).push([pieces, pside, dev]() mutable {
        enter_device(dev);
        hipStream_t ss = side_stream(pside);
        std::vector<mccnn_geometry_t*> hs;
        std::vector<int> whats;
        std::vector<PieceEntry*> live;
        bool avg = (*pieces)[0].avg;
        hipEvent_t last = nullptr;
        for (PieceEntry& pe : *pieces) {
            Geo& g = *pe.g;
            g.wait_build_issued_nothrow();
            if (g.build_rc != 0) continue;
            const int prev = mccnn_debug_wait_accounting(0);
            const int E = mccnn_geometry_edges(g.h, -1);
            mccnn_debug_wait_accounting(prev);
            if (E >= 0) g.e.store(E, std::memory_order_relaxed);
            if (E <= 0 || E > g.e_cap) continue;
            int rc = 0;
            for (int k = 0; k < 4 && !rc; ++k)
                if (pe.what & (1 << k)) rc = mccnn_geometry_attach(g.h, 1 << k, pe.base + pe.off[k], (size_t)pe.len[k]);
            if (rc) continue;   // (left unbuilt: the layer that needs a piece builds it, and reports)
            g.have |= pe.what;
            hs.push_back(g.h);
            whats.push_back(pe.what & 7);
            live.push_back(&pe);
            if (g.event) last = g.event;
        }
        int rc = 0;
        if (!hs.empty()) {
            // behind the builds (one stream, events recorded in order: the last one covers them all)
            if (last && hipStreamWaitEvent(ss, last, 0) != hipSuccess) rc = (int)hipErrorUnknown;
            if (!rc) {
                try {
                    const size_t wsb = mccnn_geometry_prebuild_batch_ws_bytes(hs.data(), whats.data(), (int)hs.size());
                    Tensor& ws = scratch(wsb, live[0]->g->buf, (void*)ss);
                    rc = mccnn_geometry_prebuild_batch(hs.data(), whats.data(), (int)hs.size(), avg ? 1 : 0, ws.data_ptr(), (size_t)ws.numel(), (void*)ss);
                } catch (const std::exception&) {
                    rc = (int)hipErrorUnknown;
                }
            }
            if (rc) fprintf(stderr, "mccnn: batch of row plans / transposed lists: error %d (the layers build what is missing)\n", rc);
            // (events also after an error: part of the batch may have been launched, and whoever frees a geometry's memory
            // orders its stream behind them -- Geo::~Geo)
            for (PieceEntry* pe : live) {
                Geo& g = *pe->g;
                if (pe->what & 1) {
                    if (!g.plan_event) g.plan_event = take_event();
                    if (hipEventRecord(g.plan_event, ss) == hipSuccess) g.plan_wait = true;
                }
                if (pe->what & 6) {
                    if (!g.tr_event) g.tr_event = take_event();
                    if (hipEventRecord(g.tr_event, ss) == hipSuccess) g.tr_wait = true;
                }
                g.pre_avg = avg ? 1 : 0;
            }
        }
        for (PieceEntry& pe : *pieces) pe.g->pieces_issued.store(1, std::memory_order_release);
    });
}

std::shared_ptr<Geo> build_geometry(const Tensor& pts, const Tensor& bids, const Tensor& centres, const Tensor& cbids,
                                    const Tensor& mn, const Tensor& mx, int64_t B, int64_t nc, double radius, bool scale_inv,
                                    double window, bool use_pdf, int64_t capacity, std::shared_ptr<Geo> grid_from,
                                    int64_t side, bool fork, bool background, std::shared_ptr<HierFuture> after,
                                    int64_t max_neighbors, int64_t sample_seed /* < 0: none */, bool point_pdf,
                                    std::shared_ptr<PointPdf> point_from /* the density of this grid and window, when it exists */,
                                    int64_t max_edges /* the edge budget of the search; 0: none */,
                                    int64_t records_avg /* >= 0: the KDE leaves the per-edge records of layers with this `avg`; -1: none */) {
    check_dev(pts, at::kFloat, "points");
    check_dev(centres, at::kFloat, "sample points");
    check_dev(bids, at::kInt, "batch ids");
    check_dev(cbids, at::kInt, "sample batch ids");
    check_dev(mn, at::kFloat, "aabb_min");
    check_dev(mx, at::kFloat, "aabb_max");
    const DevGuard device_guard((int)pts.device().index());
    const int n = (int)pts.size(0), m = (int)centres.size(0);
    if (grid_from && grid_from->grid_owner) grid_from = grid_from->grid_owner;
    TORCH_CHECK(max_neighbors >= 0 && max_neighbors <= 0x7fffffffLL, "geometry: maxNeighbors must be >= 0");
    TORCH_CHECK(max_edges >= 0 && max_edges <= 0x7fffffffLL, "geometry: maxEdges must lie in [0, 2^31)");
    TORCH_CHECK(sample_seed < 0 || ((max_neighbors > 0 || max_edges > 0) && sample_seed <= 0xffffffffLL), "geometry: sampleSeed needs a cap or a budget and lies in [0, 2^32)");
    TORCH_CHECK(!(point_pdf || point_from) || (use_pdf && max_neighbors == 0 && max_edges == 0), "geometry: a per-point density needs usePDF and an uncapped list");
    TORCH_CHECK(!point_from || (point_from->density.defined() && point_from->density.size(0) == n), "geometry: the per-point density is of another grid");
    std::shared_ptr<PointPdf> pp = point_from;
    const bool pp_ready = pp != nullptr;
    // a density that does not exist yet: allocated with the geometry's buffer (same pool, same stream), written by this build
    auto make_pp = [&](void* alloc_stream) {
        if (!point_pdf || pp) return;
        pp = std::make_shared<PointPdf>();
        pp->density = at::empty({(int64_t)n, 1}, pts.options());
        pp->counts = at::empty({(int64_t)n, 1}, pts.options().dtype(at::kInt));
        pp->alloc_stream = alloc_stream;
        pp->ev = take_event();
    };
    // the cap of the search (by value into the helper thread's job / the batch entry)
    const mccnn_neighbor_cap cap{(int)max_neighbors, sample_seed >= 0 ? 1 : 0, sample_seed >= 0 ? (unsigned)sample_seed : 0u};
    const mccnn_neighbor_budget budget{(int)max_edges};
    size_t bytes = mccnn_geometry_bytes_budget(n, m, (int)B, (int)nc, (int)capacity, grid_from ? 0 : 1, cap.max_neighbors, budget.max_edges);
    TORCH_CHECK(bytes > 0, "geometry: batch_size * num_cells^3 does not fit 32-bit keys");
    // per-edge records from the build's KDE (mccnn_geometry_want_records): behind the geometry's own pieces, in the same
    // buffer -- no block, event or stream ordering of their own
    static const bool kde_records = mccnn::debug_int("kde_records", 1) != 0;
    const bool want_records = records_avg >= 0 && kde_records && use_pdf && !point_pdf && !point_from;
    if (want_records) bytes += mccnn_geometry_records_bytes((int)capacity);
    auto g = std::make_shared<Geo>();
    g->h = mccnn_geometry_create();
    TORCH_CHECK(g->h, "mccnn_geometry_create failed");
    if (want_records) {
        check(mccnn_geometry_want_records(g->h, records_avg ? 1 : 0), "geometry_want_records");
        g->have |= 8;   // (the record buffer is there: a row plan built ahead attaches none of its own)
    }
    g->slot = take_slot();
    g->keep = {pts, bids, centres, cbids, mn, mx};
    g->grid_owner = grid_from;
    g->n = n; g->m = m; g->nc = (int)nc; g->B = (int)B; g->e_cap = capacity;
    void* stream = cur_stream(pts);
    g->alloc_stream = stream;
    // a geometry that shares another one's grid runs behind it on the same side stream
    if (side >= 0 && grid_from && grid_from->side >= 0 && grid_from->needs_wait) side = grid_from->side;
    // ... and the geometries of a batch all run on the side stream of the first one
    const bool batched = side >= 0 && t_geo_batch.active;
    const int asked_side = side >= 0 ? (int)(((side % kSideStreams) + kSideStreams) % kSideStreams) : -1;
    if (batched) {
        if (t_geo_batch.side < 0) { t_geo_batch.side = (int)(((side % kSideStreams) + kSideStreams) % kSideStreams); t_geo_batch.background = background; }
        side = t_geo_batch.side;
    }
    // Everything this build reads is the adopted prefetched hierarchy `after` (its points, batch ids, boxes -- and a grid
    // that was itself built this way): the build then waits for THAT, takes its memory from its own stream's pool and
    // starts now, not behind what the calling stream holds (Geo::own_pool).
    static const bool own_pools = mccnn::debug_int("geo_own_pool", 1) != 0;
    hipEvent_t ready = (side >= 0 && own_pools && Issuer::enabled()) ? hierarchy_ready_event(after) : nullptr;
    if (ready && grid_from && !grid_from->own_pool) ready = nullptr;
    if (ready && pp && pp->alloc_stream != (void*)side_stream((int)side)) {
        // (a density of another pool: this build reads memory the allocator knows from another stream -- fork like any other)
        bool pool_side = false;
        for (int k = 0; k < kSideStreams; ++k) pool_side = pool_side || pp->alloc_stream == (void*)side_stream(k);
        if (!pool_side) ready = nullptr;
    }
    // ... and only then: an input that is NOT the hierarchy's own memory (a re-made-contiguous copy of a level, a tensor
    // the caller produced on its stream) is ordered by the calling stream alone -- such a build forks behind it like any other
    if (ready)
        for (const Tensor* t : {&pts, &bids, &centres, &cbids, &mn, &mx})
            if (!hierarchy_owns(after, *t)) { ready = nullptr; break; }
    // (a build that takes the fork path after one that did not: the caller's fork=false refers to a record that was skipped)
    static thread_local bool fork_skipped = false;
    if (ready && side_stream((int)side)) {
        hipStream_t ss = side_stream((int)side);
        if (fork) fork_skipped = true;
        {
            const c10::hip::HIPStreamGuardMasqueradingAsCUDA own(as_torch_stream((void*)ss, (int)pts.device().index()));
            if (batched) g->buf = arena_take(0, (int64_t)bytes, pts);
            if (!g->buf.defined()) g->buf = at::empty({(int64_t)bytes}, pts.options().dtype(at::kByte));
            make_pp((void*)ss);
        }
        g->own_pool = true;
        g->caller_stream = stream;
        g->has_caller = true;
        g->alloc_stream = (void*)ss;
        hip_check(hipStreamWaitEvent(ss, ready, 0), "hipStreamWaitEvent");
        const int sk = (int)(((side % kSideStreams) + kSideStreams) % kSideStreams);
        if (grid_from && grid_from->event && grid_from->side != sk) {
            grid_from->wait_issued();
            hip_check(hipStreamWaitEvent(ss, grid_from->event, 0), "hipStreamWaitEvent");
        }
        g->side = sk;
        stream = ss;
    } else if (side >= 0) {
        g->buf = at::empty({(int64_t)bytes}, pts.options().dtype(at::kByte));
        make_pp(stream);
        hipStream_t ss = side_stream((int)side);
        if (ss) {
            // the side stream starts behind everything the calling stream held at the last fork (the point hierarchy;
            // whatever used the memory the allocator hands out from there on). Only the stream that gets work waits:
            // a wait packet on an idle queue keeps that queue in the command processor's rotation for nothing
            static thread_local hipEvent_t fork_ev = nullptr;
            if (!fork_ev) {
                hip_check(hipEventCreateWithFlags(&fork_ev, hipEventDisableTiming), "hipEventCreate");
                fork = true;
            }
            if (fork || fork_skipped) hip_check(hipEventRecord(fork_ev, (hipStream_t)stream), "hipEventRecord");
            fork_skipped = false;
            hip_check(hipStreamWaitEvent(ss, fork_ev, 0), "hipStreamWaitEvent");
            // (a grid owner on another side stream -- its build has been joined by the caller's stream already, or it
            // would have pulled this build onto its own stream above: order this stream behind it without consuming the
            // owner's one-time join)
            if (grid_from && grid_from->event && grid_from->side != (int)(((side % kSideStreams) + kSideStreams) % kSideStreams)) {
                grid_from->wait_issued();
                hip_check(hipStreamWaitEvent(ss, grid_from->event, 0), "hipStreamWaitEvent");
            }
            g->side = (int)(((side % kSideStreams) + kSideStreams) % kSideStreams);
            stream = ss;
        }
    } else {
        g->buf = at::empty({(int64_t)bytes}, pts.options().dtype(at::kByte));
        make_pp(stream);
        if (grid_from) grid_from->join(stream);
    }
    // the density: its writer runs on `stream`; a sharer's stream is ordered behind the sweep (an event wait, when the
    // streams differ) and made known to the allocator of the density's pool
    mccnn_point_pdf point{nullptr, nullptr, 0};
    if (pp) {
        g->pp = pp;
        if (!pp_ready) pp->write_stream = stream;
        pp->order(stream);
        point = mccnn_point_pdf{pp->density.data_ptr<float>(), pp->counts.data_ptr<int>(), pp_ready ? 1 : 0};
    }
    const bool writes_point = pp && !pp_ready;
    if (g->side >= 0 && Issuer::enabled()) {
        // the helper thread issues the launches and records the event; whoever touches the geometry waits for `issued`
        g->event = take_event();
        g->needs_wait = true;
        g->issued.store(0, std::memory_order_release);
        const float* p0 = pts.data_ptr<float>();
        const int* p1 = bids.data_ptr<int>();
        const float* p2 = centres.data_ptr<float>();
        const int* p3 = cbids.data_ptr<int>();
        const float* p4 = mn.data_ptr<float>();
        const float* p5 = mx.data_ptr<float>();
        void* bufp = g->buf.data_ptr();
        int* slotp = g->slot.data_ptr<int>();
        const int iB = (int)B, inc = (int)nc, icap = (int)capacity, isi = scale_inv ? 1 : 0, ipdf = use_pdf ? 1 : 0;
        const float fr = (float)radius, fw = (float)window;
        const int dev = (int)pts.device().index();
        if (batched && stream == (void*)side_stream(t_geo_batch.side)) {   // recorded: end_geometry_batch() issues the list
            BatchEntry e;
            e.g = g;
            e.grid_from = grid_from;
            e.req = mccnn_geometry_request{g->h, p0, p1, n, p2, p3, m, p4, p5, iB, inc, fr, isi, fw, ipdf, icap,
                                           grid_from ? grid_from->h : nullptr, bufp, bytes, slotp};
            e.cap = cap;
            e.point = point;
            e.budget = budget;
            e.writes_point = writes_point;
            t_geo_batch.entries.push_back(std::move(e));
            g->plan_side = asked_side;   // the pieces built ahead keep the spread over the side streams the builds gave up
            return g;
        }
        Issuer::get().push([g, grid_from, p0, p1, p2, p3, p4, p5, bufp, slotp, n, m, iB, inc, icap, isi, ipdf, fr, fw, bytes, stream, background, dev, cap, point, writes_point, budget] {
            enter_device(dev);
            if (grid_from) grid_from->wait_issued_nothrow();
            // background: these launches run beside kernels a step waits for (the convolutions of the current batch) --
            // the search kernels then hold back (mccnn_background_launches, thread-local: set on THIS thread)
            const int prev = background ? mccnn_background_launches(1) : 0;
            int rc = mccnn_geometry_build_budget(g->h, p0, p1, n, p2, p3, m, p4, p5, iB, inc, fr, isi, fw, ipdf, icap,
                                                 grid_from ? grid_from->h : nullptr, bufp, bytes, slotp, stream, &cap, &point, &budget);
            if (background) mccnn_background_launches(prev);
            if (writes_point) g->pp->mark(stream);
            if (rc == 0 && hipEventRecord(g->event, (hipStream_t)stream) != hipSuccess) rc = (int)hipErrorUnknown;
            g->build_rc = rc;
            g->issued.store(1, std::memory_order_release);
        });
        return g;
    }
    if (grid_from) grid_from->wait_issued();
    const int prev_bg = (background && g->side >= 0) ? mccnn_background_launches(1) : 0;
    struct Restore {
        bool on; int prev;
        ~Restore() { if (on) mccnn_background_launches(prev); }
    } restore{background && g->side >= 0, prev_bg};
    const int build_rc = mccnn_geometry_build_budget(g->h, pts.data_ptr<float>(), bids.data_ptr<int>(), n, centres.data_ptr<float>(),
                                                    cbids.data_ptr<int>(), m, mn.data_ptr<float>(), mx.data_ptr<float>(), (int)B, (int)nc,
                                                    (float)radius, scale_inv ? 1 : 0, (float)window, use_pdf ? 1 : 0, (int)capacity,
                                                    grid_from ? grid_from->h : nullptr, g->buf.data_ptr(), bytes,
                                                    g->slot.data_ptr<int>(), stream, &cap, &point, &budget);
    if (writes_point) pp->mark(stream);
    check(build_rc, "geometry_build");
    if (g->side >= 0) {
        g->event = take_event();
        hip_check(hipEventRecord(g->event, (hipStream_t)stream), "hipEventRecord");
        g->needs_wait = true;
    }
    return g;
}

// Pieces of a geometry whose build has just been queued on a side stream (learned prefetch: the layers of the previous
// step over this list used them): the buffers are allocated HERE -- on the calling thread and its stream, sized by bounds
// that hold for any list within the capacity -- and the helper thread attaches and issues them behind the build once the
// edge total has arrived. The calling thread neither waits for the total nor issues the ~20 launches of a list's plans.
void prebuild_async(std::shared_ptr<Geo> g, int what, bool avg) {
    if (!g || g->side < 0 || !Issuer::enabled() || g->e_cap <= 0) return;
    const DevGuard device_guard((int)g->buf.device().index());
    if (what & 3) what |= 8;
    if (what & 2) what |= 4;
    what &= 15 & ~g->have;
    if (!what) return;
    long long off[4] = {0, 0, 0, 0}, len[4] = {0, 0, 0, 0}, total = 0, wsb = 256;
    for (int k = 0; k < 4; ++k) {
        if (!(what & (1 << k))) continue;
        long long b = 0, w = 0;
        check(mccnn_geometry_piece_bound(g->n, g->m, (int)g->e_cap, 1 << k, &b, &w), "geometry_piece_bound");
        off[k] = total;
        len[k] = b;
        total += (b + 255) / 256 * 256;
        if (w > wsb) wsb = w;
    }
    // a batched geometry: its pieces join the batch too, on ONE side stream (the next one after the builds')
    const bool batched = t_geo_batch.active && t_geo_batch.side >= 0 && g->plan_side >= 0;
    if (batched) g->plan_side = (t_geo_batch.side + 1) % kSideStreams;
    const bool other = g->plan_side >= 0 && g->plan_side != g->side;   // (a batch build: pieces on another side stream, behind the build's event)
    hipStream_t ss = side_stream(other ? g->plan_side : g->side);
    Tensor block;
    if (g->own_pool) {
        const c10::hip::HIPStreamGuardMasqueradingAsCUDA own(as_torch_stream((void*)ss, (int)g->buf.device().index()));
        if (batched) block = arena_take(1, (int64_t)total, g->buf);
        if (!block.defined()) block = at::empty({(int64_t)total}, g->buf.options());
    } else {
        block = at::empty({(int64_t)total}, g->buf.options());
    }
    g->attached.push_back(block);
    g->pieces_issued.store(0, std::memory_order_release);
    char* base = (char*)block.data_ptr();
    Tensor like = g->buf;
    if (batched) {
        PieceEntry pe;
        pe.g = g; pe.what = what; pe.avg = avg; pe.base = base;
        for (int k = 0; k < 4; ++k) { pe.off[k] = off[k]; pe.len[k] = len[k]; }
        t_geo_batch.pieces.push_back(std::move(pe));
        return;
    }
    Issuer::get(2).push([g, what, avg, base, off, len, wsb, ss, like, other]() mutable {
        enter_device((int)like.device().index());
        g->wait_build_issued_nothrow();
        if (g->build_rc == 0 && other && g->event && hipStreamWaitEvent(ss, g->event, 0) != hipSuccess) g->build_rc = (int)hipErrorUnknown;
        if (g->build_rc == 0) {
            const int prev = mccnn_debug_wait_accounting(0);
            const int E = mccnn_geometry_edges(g->h, -1);
            mccnn_debug_wait_accounting(prev);
            if (E >= 0) g->e.store(E, std::memory_order_relaxed);
            if (E > 0 && E <= g->e_cap) {
                int rc = 0;
                for (int k = 0; k < 4 && !rc; ++k)
                    if (what & (1 << k)) rc = mccnn_geometry_attach(g->h, 1 << k, base + off[k], (size_t)len[k]);
                if (!rc) {
                    g->have |= what;
                    try {
                        Tensor& ws = scratch((size_t)wsb, like, (void*)ss);
                        rc = g->issue_pieces(what & 7, avg, ss, ws.data_ptr(), (size_t)ws.numel());
                    } catch (const std::exception&) {
                        rc = (int)hipErrorUnknown;
                    }
                }
                // (a failure here leaves the pieces attached but unbuilt: the layer that needs one builds it, and reports)
            }
        }
        g->pieces_issued.store(1, std::memory_order_release);
    });
}

struct Layer {
    int fin, fout, combin, avg, bf16, flags;
};

// mccnn_conv_prepare + the attachments it asks for; -> scratch bytes, saved bytes
void prepare(Geo& g, const Tensor& feats, const Layer& L, int backward, int flags, long long& ws_bytes, long long& saved_bytes) {
    int mask = 0, edges = 0;
    long long need[4] = {0, 0, 0, 0};
    int rc = mccnn_conv_prepare(g.h, feats.data_ptr(), L.fin, L.fout, L.combin, L.bf16, backward, flags, &mask, need, &ws_bytes,
                                &saved_bytes, &edges);
    if (rc == MCCNN_E_CAPACITY) {
        g.e = edges;
        throw CapacityError(edges);
    }
    check(rc, "conv_prepare");
    g.e = edges;
    for (int k = 0; k < 4 && mask; ++k) {
        const int bit = 1 << k;
        if (!(mask & bit)) continue;
        Tensor t = at::empty({(int64_t)(need[k] > 256 ? need[k] : 256)}, feats.options().dtype(at::kByte));
        check(mccnn_geometry_attach(g.h, bit, t.data_ptr(), (size_t)t.numel()), "geometry_attach");
        g.attached.push_back(std::move(t));
        g.have |= bit;
    }
}

// host-time census of the layer calls (debug_times(): ns and calls per section; cheap enough to stay compiled in)
enum { T_FWD = 0, T_FWD_LIB, T_FWD_ALLOC, T_BWD, T_BWD_LIB, T_BWD_ALLOC, T_BWD_VIEWS, T_BWD_JOIN, T_N };
std::atomic<long long> g_t_ns[T_N], g_t_calls[T_N];
struct Tick {
    int k;
    std::chrono::steady_clock::time_point t0;
    explicit Tick(int k_) : k(k_), t0(std::chrono::steady_clock::now()) {}
    ~Tick() {
        g_t_ns[k].fetch_add(std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count(), std::memory_order_relaxed);
        g_t_calls[k].fetch_add(1, std::memory_order_relaxed);
    }
};

struct ConvBackward : public torch::autograd::Node {
    std::shared_ptr<Geo> geo;
    // the seven inputs, held as plain tensors with the version each had in the forward pass (they are INPUTS of this node,
    // so holding them makes no cycle; SavedVariable::unpack builds a fresh Variable per tensor and call, ~5 us per node --
    // what it guards against, an input modified in place since the forward pass, is checked here directly)
    Tensor feats_, w1_, b1_, w2_, b2_, w3_, b3_;
    uint32_t versions[7] = {0, 0, 0, 0, 0, 0, 0};
    Tensor rows_;   // bf16 rows that did not start on a 16-byte boundary: the aligned copy the forward pass read (conv())
    Tensor saved;
    Layer L;

    torch::autograd::variable_list apply(torch::autograd::variable_list&& grads) override {
        const Tick tick_all(T_BWD);
        TORCH_CHECK(geo && feats_.defined(), "MC convolution: backward through a graph whose buffers have been freed (retain_graph=True?)");
        const DevGuard device_guard((int)geo->buf.device().index());
        const Tensor &feats = rows_.defined() ? rows_ : feats_, &w1 = w1_, &b1 = b1_, &w2 = w2_, &b2 = b2_, &w3 = w3_, &b3 = b3_;
        {
            const Tensor* in[7] = {&feats_, &w1_, &b1_, &w2_, &b2_, &w3_, &b3_};
            for (int k = 0; k < 7; ++k)
                TORCH_CHECK(in[k]->_version() == versions[k],
                            "one of the variables needed for gradient computation has been modified by an inplace operation "
                            "(MC convolution input ", k, ")");
        }
        Tensor og = grads[0];
        if (!og.defined()) og = at::zeros({geo->m, L.combin ? L.fout : L.fin}, feats.options());
        if (!og.is_contiguous()) og = og.contiguous();
        if (og.scalar_type() != feats.scalar_type()) og = og.to(feats.scalar_type());
        // (bf16 rows: the kernels move 16-byte pieces; an out-gradient that starts anywhere else -- a view into a larger
        // buffer -- is copied into an allocation of its own. f32 rows stay where they are: scalar kernels exist for them)
        if (L.bf16 && (reinterpret_cast<uintptr_t>(og.data_ptr()) & 15) != 0) og = og.clone(at::MemoryFormat::Contiguous);
        int flags = L.flags;
        // several layers share this neighbour list: its transposed form is built once and the feature gradient of combin
        // layers with 2..4 input features is gathered through it in a fixed order (bit-reproducible) instead of added
        // with float atomics; a bare single call keeps the atomics (the list would cost more than they do)
        if (geo->uses > 1) flags |= MCCNN_CONV_DETERMINISTIC;
        { const Tick tj(T_BWD_JOIN); geo->join(cur_stream(feats), true); }
        long long wsb = 0, svb = 0;
        prepare(*geo, feats, L, 1, flags, wsb, svb);
        Tensor fg;
        Tensor gflat;
        // the six MLP gradients: consecutive slices of ONE buffer in the order the builder creates the variables (a
        // data-parallel step all-reduces that buffer as it is, dist.GradBucket)
        const int64_t n1 = w1.numel(), n2 = b1.numel(), n3 = w2.numel(), n4 = b2.numel(), n5 = w3.numel(), n6 = b3.numel();
        {
            const Tick ta(T_BWD_ALLOC);
            fg = at::empty_like(feats);
            gflat = at::empty({n1 + n2 + n3 + n4 + n5 + n6}, w1.options());
        }
        float* base = gflat.data_ptr<float>();
        void* st = cur_stream(feats);
        Tensor& ws = scratch((size_t)wsb, feats, st);
        {
        const Tick tl(T_BWD_LIB);
        check(mccnn_conv_backward(geo->h, feats.data_ptr(), saved.defined() ? saved.data_ptr() : nullptr,
                                  saved.defined() ? (size_t)saved.numel() : 0, og.data_ptr(), L.fin, L.fout, L.combin, L.avg,
                                  L.bf16, flags, w1.data_ptr<float>(), b1.data_ptr<float>(), w2.data_ptr<float>(),
                                  b2.data_ptr<float>(), w3.data_ptr<float>(), b3.data_ptr<float>(), fg.data_ptr(), base,
                                  base + n1, base + n1 + n2, base + n1 + n2 + n3, base + n1 + n2 + n3 + n4,
                                  base + n1 + n2 + n3 + n4 + n5, ws.data_ptr(), (size_t)ws.numel(), st),
              "conv_backward");
        }
        const Tick tv(T_BWD_VIEWS);
        int64_t o = 0;
        auto piece = [&](int64_t cnt, const Tensor& like) {
            Tensor t = gflat.as_strided(like.sizes(), like.strides(), o);   // (contiguous variables: checked in conv())
            o += cnt;
            return t;
        };
        torch::autograd::variable_list out(7);
        out[0] = fg;
        out[1] = piece(n1, w1); out[2] = piece(n2, b1); out[3] = piece(n3, w2); out[4] = piece(n4, b2);
        out[5] = piece(n5, w3); out[6] = piece(n6, b3);
        return out;
    }

    void release_variables() override {
        feats_.reset(); w1_.reset(); b1_.reset(); w2_.reset(); b2_.reset(); w3_.reset(); b3_.reset();
        rows_.reset();
        saved.reset();
        geo.reset();
    }
};

// One MC convolution over `geo` (SpatialConv with sort_features folded in, MCConvModuleSrc:35-45,70-81): feats are the
// rows of the UNSORTED input points ([n, Fin] f32, or bf16 for depth-wise layers); the kernel-MLP tensors in any shape
// over the reference's flat layout.
Tensor conv(std::shared_ptr<Geo> geo, const Tensor& feats_in, const Tensor& w1, const Tensor& b1, const Tensor& w2,
            const Tensor& b2, const Tensor& w3, const Tensor& b3, int64_t fout, bool combin, bool avg, bool deterministic) {
    TORCH_CHECK(geo && geo->h, "conv: no geometry");
    const DevGuard device_guard((int)feats_in.device().index());
    TORCH_CHECK(feats_in.defined() && feats_in.is_cuda() && feats_in.dim() == 2 && feats_in.size(0) == geo->n && feats_in.is_contiguous(),
                "SpatialConvOp expects as feature inputs the following dimensions (numPoints, numFeatures)");
    const bool bf = feats_in.scalar_type() == at::kBFloat16;
    TORCH_CHECK(bf || feats_in.scalar_type() == at::kFloat, "features must be float32 or bfloat16");
    for (const Tensor* t : {&w1, &b1, &w2, &b2, &w3, &b3}) check_dev(*t, at::kFloat, "kernel-MLP tensor");
    Layer L;
    L.fin = (int)feats_in.size(1); L.fout = (int)fout; L.combin = combin ? 1 : 0; L.avg = avg ? 1 : 0; L.bf16 = bf ? 1 : 0;
    const bool need_grad = at::GradMode::is_enabled() &&
                           (feats_in.requires_grad() || w1.requires_grad() || b1.requires_grad() || w2.requires_grad() ||
                            b2.requires_grad() || w3.requires_grad() || b3.requires_grad());
    // MCCNN_CONV_DETERMINISTIC: the caller asks for bit-reproducible feature gradients (combin layers with 2..4 input features gather them
    // through the transposed list instead of adding them with float atomics)
    L.flags = (need_grad ? MCCNN_CONV_KEEP_STATE : 0) | (deterministic ? MCCNN_CONV_DETERMINISTIC : 0);
    Tensor out, saved;
    // bf16 rows that do not start on a 16-byte boundary (a view into a larger buffer): the bf16 kernels move 16-byte pieces
    // and the permutes see the rows as 32-bit words, so such rows are copied into an allocation of their own, which both
    // passes read. f32 rows stay where they are: the executor leaves the in-place mode and the vector kernels by itself.
    Tensor rows_copy;
    const Tick tick_all(T_FWD);
    {
        at::AutoDispatchBelowADInplaceOrView guard;
        if (bf && (reinterpret_cast<uintptr_t>(feats_in.data_ptr()) & 15) != 0) rows_copy = feats_in.detach().clone(at::MemoryFormat::Contiguous);
        const Tensor& feats = rows_copy.defined() ? rows_copy : feats_in;
        geo->join(cur_stream(feats), geo->pre_avg != L.avg);
        if (geo->grid_owner) geo->grid_owner->join(cur_stream(feats));
        // MCCNN_CONV_READS_RECORDS: the geometry holds the per-edge records of this layer (its KDE wrote them): read in both passes, kept by neither
        if (L.fin == 1 && L.combin && mccnn_conv_uses_records(geo->h, L.fin, L.fout, L.combin, L.avg)) L.flags |= MCCNN_CONV_READS_RECORDS;
        long long wsb = 0, svb = 0;
        prepare(*geo, feats, L, 0, L.flags, wsb, svb);
        {
            const Tick ta(T_FWD_ALLOC);
            out = at::empty({geo->m, combin ? fout : (int64_t)L.fin}, feats.options());
            if (svb > 0) saved = at::empty({(int64_t)svb}, feats.options().dtype(at::kByte));
        }
        void* st = cur_stream(feats);
        Tensor& ws = scratch((size_t)wsb, feats, st);
        const Tick tl(T_FWD_LIB);
        check(mccnn_conv_forward(geo->h, feats.data_ptr(), L.fin, L.fout, L.combin, L.avg, L.bf16, L.flags, w1.data_ptr<float>(),
                                 b1.data_ptr<float>(), w2.data_ptr<float>(), b2.data_ptr<float>(), w3.data_ptr<float>(),
                                 b3.data_ptr<float>(), out.data_ptr(), saved.defined() ? saved.data_ptr() : nullptr,
                                 (size_t)svb, ws.data_ptr(), (size_t)ws.numel(), st),
              "conv_forward");
    }
    if (need_grad) {
        auto node = std::shared_ptr<ConvBackward>(new ConvBackward(), torch::autograd::deleteNode);
        node->set_next_edges(torch::autograd::collect_next_edges(feats_in, w1, b1, w2, b2, w3, b3));
        node->geo = geo;
        node->rows_ = rows_copy;
        node->feats_ = feats_in; node->w1_ = w1; node->b1_ = b1; node->w2_ = w2; node->b2_ = b2; node->w3_ = w3; node->b3_ = b3;
        {
            const Tensor* in[7] = {&feats_in, &w1, &b1, &w2, &b2, &w3, &b3};
            for (int k = 0; k < 7; ++k) node->versions[k] = in[k]->_version();
        }
        node->saved = saved;
        node->L = L;
        torch::autograd::set_history(out, node);
    }
    return out;
}

// ComputeAabb through the extension (aabb_gpu.cc:22-86): the op a hierarchy without a prefetch request starts with, every
// step -- one C++ call instead of the ctypes op (two allocations, a workspace look-up, ten argument conversions).
std::vector<Tensor> compute_aabb(const Tensor& pts, const Tensor& bids, int64_t B, bool scale_inv) {
    check_dev(pts, at::kFloat, "points");
    check_dev(bids, at::kInt, "batch ids");
    TORCH_CHECK(B > 0, "ComputeAabbOp expects a positive batch size");
    const DevGuard device_guard((int)pts.device().index());
    Tensor mn = at::empty({B, 3}, pts.options()), mx = at::empty({B, 3}, pts.options());
    void* st = cur_stream(pts);
    Tensor& ws = scratch(mccnn_compute_aabb_workspace_bytes((int)B), pts, st);
    check(mccnn_compute_aabb(pts.data_ptr<float>(), bids.data_ptr<int>(), (int)pts.size(0), (int)B, scale_inv ? 1 : 0, mn.data_ptr<float>(),
                             mx.data_ptr<float>(), ws.data_ptr(), (size_t)ws.numel(), st),
          "compute_aabb");
    return {mn, mx};
}

std::atomic<long long> g_wait_ns{0};  // host time spent waiting for the level sizes (diagnostics: wait_ns())
void count_wait(std::chrono::steady_clock::time_point t0) {
    if (t_helper_thread) return;   // (only the calling side's waits: a helper thread waiting is the point of having it)
    g_wait_ns.fetch_add(std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count(),
                        std::memory_order_relaxed);
}

// Geometry of ALL levels of a point hierarchy (MCConvBuilder.py:101-128 per level: sort_points_step1/2 -> poisson_sampling
// -> transform_indexs) with device-side point counts and ONE read-back of the level sizes at the end: the C++ form of
// MCConvModule.point_hierarchy_levels (one library call per level, two allocations, no Python in between).
// -> per level (sampledPts [S,3], sampledBatchIds [S,1], sampledIndexs [S], transformedIndexs [S]); an empty vector when a
// wait of the single-launch Poisson kernel timed out (the caller then runs the op-by-op chain).
std::vector<std::vector<Tensor>> hierarchy_levels(const Tensor& pts, const Tensor& bids, const Tensor& mn, const Tensor& mx,
                                                  const std::vector<double>& radii, const std::vector<int64_t>& ncs,
                                                  int64_t B, bool scale_inv, int64_t pmode) {
    check_dev(pts, at::kFloat, "points");
    check_dev(bids, at::kInt, "batch ids");
    check_dev(mn, at::kFloat, "aabb_min");
    check_dev(mx, at::kFloat, "aabb_max");
    const DevGuard device_guard((int)pts.device().index());
    const int L = (int)radii.size();
    const int cap = (int)pts.size(0);
    TORCH_CHECK(L > 0 && (int)ncs.size() == L && cap > 0, "hierarchy_levels: bad arguments");
    void* st = cur_stream(pts);
    auto iopt = pts.options().dtype(at::kInt);
    Tensor sizes = at::empty({L + 1}, iopt);
    hip_check(hipMemcpyAsync(sizes.data_ptr(), &cap, sizeof(int), hipMemcpyHostToDevice, (hipStream_t)st), "hipMemcpyAsync");
    const int64_t ca = (cap + 63) / 64 * 64;  // 256-byte aligned pieces (the cell table is written as int2)
    std::vector<Tensor> ints(L), flts(L);
    const float* cur_pts = pts.data_ptr<float>();
    const int* cur_bids = bids.data_ptr<int>();
    int* sz = sizes.data_ptr<int>();
    for (int l = 0; l < L; ++l) {
        const int nc = (int)ncs[l];
        const size_t wsb = mccnn_hierarchy_level_workspace_bytes(cap, (int)B, nc);
        TORCH_CHECK(wsb > 0, "PointHierarchy: batch_size * num_cells^3 does not fit 32-bit keys");
        Tensor& ws = scratch(wsb, pts, st);
        // index_new_pos | sorted batch ids | oB | oI | ti | cell table          and          sorted points | sampled points
        ints[l] = at::empty({5 * ca + 2 * B * nc * nc * nc}, iopt);
        flts[l] = at::empty({6 * ca}, pts.options());
        int* bi = ints[l].data_ptr<int>();
        float* bf = flts[l].data_ptr<float>();
        check(mccnn_hierarchy_level(cur_pts, cur_bids, mn.data_ptr<float>(), mx.data_ptr<float>(), cap, sz + l, (int)B, nc,
                                    (float)radii[l], scale_inv ? 1 : 0, (int)pmode, bi, bf, bi + ca, bi + 5 * ca, bf + 3 * ca,
                                    bi + 2 * ca, bi + 3 * ca, bi + 4 * ca, sz + l + 1, ws.data_ptr(), (size_t)ws.numel(), st),
              "hierarchy_level");
        cur_pts = bf + 3 * ca;
        cur_bids = bi + 2 * ca;
    }
    // the ONE read-back: every level's sample count
    static thread_local Tensor host;
    if (!host.defined() || host.numel() < L + 1) host = at::empty({L + 65}, at::TensorOptions().dtype(at::kInt).pinned_memory(true));
    hip_check(hipMemcpyAsync(host.data_ptr(), sz, (size_t)(L + 1) * sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)st), "hipMemcpyAsync");
    {
        const auto t0 = std::chrono::steady_clock::now();
        hip_check(hipStreamSynchronize((hipStream_t)st), "hipStreamSynchronize");
        g_wait_ns.fetch_add(std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count(),
                            std::memory_order_relaxed);
    }
    const int* hs = host.data_ptr<int>();
    std::vector<std::vector<Tensor>> out;
    for (int l = 1; l <= L; ++l)
        if (hs[l] < 0) return out;
    for (int l = 0; l < L; ++l) {
        const int64_t sN = hs[l + 1];
        Tensor oP = flts[l].narrow(0, 3 * ca, 3 * sN).view({sN, 3});
        Tensor oB = ints[l].narrow(0, 2 * ca, sN).view({sN, 1});
        Tensor oI = ints[l].narrow(0, 3 * ca, sN);
        Tensor ti = ints[l].narrow(0, 4 * ca, sN);
        out.push_back({oP, oB, oI, ti});
    }
    return out;
}


// ---- GetSampledFeatures (+Grad), MCConvModuleSrc:63-68: out[i, :] = feats[idx[i], :]; the gradient scatters into zeros.
// The C++ form of MCConvModule.get_sampled_features: a hierarchy gathers the feature rows of every level, one call each.
struct GatherBackward : public torch::autograd::Node {
    Tensor idx;
    int64_t n = 0;
    torch::autograd::variable_list apply(torch::autograd::variable_list&& grads) override {
        Tensor g = grads[0];
        TORCH_CHECK(g.defined() && idx.defined(), "GetSampledFeaturesGrad: no gradient / released buffers");
        if (!g.is_contiguous()) g = g.contiguous();
        const DevGuard device_guard((int)g.device().index());
        const int64_t words = g.size(1) * (int64_t)g.element_size() / 4;
        Tensor out = at::empty({n, g.size(1)}, g.options());
        check(mccnn_permute_scatter((const float*)g.data_ptr(), idx.data_ptr<int>(), (int)g.size(0), (int)words,
                                    (float*)out.data_ptr(), (int)n, 1, cur_stream(g)),
              "permute_scatter");
        return {out};
    }
    void release_variables() override { idx.reset(); }
};

Tensor sampled_features(const Tensor& idx, const Tensor& feats) {
    check_dev(idx, at::kInt, "sampled indexs");
    TORCH_CHECK(idx.dim() == 1, "GetSampledFeaturesOp expects indexs with the following dimensions (numSamples)");
    TORCH_CHECK(feats.defined() && feats.is_cuda() && feats.dim() == 2 && feats.size(1) > 0 && feats.is_contiguous() &&
                    (feats.scalar_type() == at::kFloat || (feats.scalar_type() == at::kBFloat16 && feats.size(1) % 2 == 0)),
                "GetSampledFeaturesOp expects features with dimensions (numPoints, numFeatures)");
    const DevGuard device_guard((int)feats.device().index());
    const int64_t words = feats.size(1) * (int64_t)feats.element_size() / 4;
    Tensor out;
    {
        at::AutoDispatchBelowADInplaceOrView guard;
        out = at::empty({idx.size(0), feats.size(1)}, feats.options());
        check(mccnn_permute_gather((const float*)feats.data_ptr(), idx.data_ptr<int>(), (int)idx.size(0), (int)words,
                                   (float*)out.data_ptr(), cur_stream(feats)),
              "permute_gather");
    }
    if (at::GradMode::is_enabled() && feats.requires_grad()) {
        auto node = std::shared_ptr<GatherBackward>(new GatherBackward(), torch::autograd::deleteNode);
        node->set_next_edges(torch::autograd::collect_next_edges(feats));
        node->idx = idx;
        node->n = feats.size(0);
        torch::autograd::set_history(out, node);
    }
    return out;
}

// ---- the dense glue as one op (mccnn_bn_act_fwd_rows / _bwd_rows): y = drop(act(bn(x))), the C++ form of
// dense_glue.bn_relu_dropout -- the same library calls with the same arguments, so the same bytes; the autograd node is
// here, so a block costs the host one Python -> C++ call forward and none backward. x and y are each f32 or bf16 rows:
// dy has y's type, dx x's. bf16 rows that do not start on a 16-byte boundary are copied where they enter, as the
// convolutions do.
inline bool is_bf16(const Tensor& t) { return t.scalar_type() == at::kBFloat16; }
inline Tensor bf16_rows_aligned(const Tensor& t) {
    if (is_bf16(t) && (reinterpret_cast<uintptr_t>(t.data_ptr()) & 15) != 0) return t.detach().clone(at::MemoryFormat::Contiguous);
    return t;
}
// What the backward of a glue node (this one, LinearBnBackward) does before it computes: its buffers still there (`alive`),
// no double backward, no input changed in place since the forward -> dy as the library reads it: zeros of `like`'s shape
// where autograd hands none over, y's type, contiguous. op: the op's name in the messages.
Tensor glue_grad_in(const char* op, bool alive, Tensor gy, std::initializer_list<const Tensor*> in, const uint32_t* versions,
                    const Tensor& like, bool y_bf16) {
    TORCH_CHECK(alive, op, ": backward through a graph whose buffers have been freed (retain_graph=True?)");
    TORCH_CHECK(!(at::GradMode::is_enabled() && gy.defined() && gy.requires_grad()), op, " is differentiable once: no double backward");
    int k = 0;
    for (const Tensor* t : in) {
        TORCH_CHECK(t->_version() == versions[k],
                    "one of the variables needed for gradient computation has been modified by an inplace operation (", op, " input ", k,
                    ")");
        ++k;
    }
    const at::ScalarType yt = y_bf16 ? at::kBFloat16 : at::kFloat;
    if (!gy.defined()) gy = at::zeros(like.sizes(), like.options().dtype(yt));
    if (gy.scalar_type() != yt) gy = gy.to(yt);
    if (!gy.is_contiguous()) gy = gy.contiguous();
    return gy;
}

struct BnActBackward : public torch::autograd::Node {
    Tensor x_, gamma_, beta_, saved;
    bool y_bf16 = false;
    uint32_t versions[3] = {0, 0, 0};
    int relu = 1;
    unsigned long long thr = 0;
    float scale = 1.f;
    unsigned seed = 0;

    torch::autograd::variable_list apply(torch::autograd::variable_list&& grads) override {
        const Tensor gy = bf16_rows_aligned(glue_grad_in("bn_relu_drop", x_.defined() && saved.defined(), grads[0], {&x_, &gamma_, &beta_},
                                                         versions, x_, y_bf16));
        const DevGuard device_guard((int)x_.device().index());
        const int n = (int)x_.size(0), c = (int)x_.size(1);
        const bool want_dx = task_should_compute_output(0);
        Tensor dx;
        if (want_dx) dx = at::empty_like(x_);
        Tensor dgb = at::empty({2, (int64_t)c}, gamma_.options());
        void* st = cur_stream(x_);
        Tensor& ws = scratch(mccnn_bn_act_workspace_bytes(n, c), x_, st);
        check(mccnn_bn_act_bwd_rows(x_.data_ptr(), is_bf16(x_) ? 1 : 0, gy.data_ptr(), y_bf16 ? 1 : 0, n, c, gamma_.data_ptr<float>(),
                                    beta_.data_ptr<float>(), saved.data_ptr<float>(), relu, thr, scale, seed,
                                    want_dx ? dx.data_ptr() : nullptr, dgb.data_ptr<float>(), dgb.data_ptr<float>() + c, ws.data_ptr(),
                                    (size_t)ws.numel(), st),
              "bn_relu_dropout_grad");
        torch::autograd::variable_list out(3);
        out[0] = dx;
        if (task_should_compute_output(1)) out[1] = dgb.select(0, 0);
        if (task_should_compute_output(2)) out[2] = dgb.select(0, 1);
        return out;
    }
    void release_variables() override { x_.reset(); gamma_.reset(); beta_.reset(); saved.reset(); }
};

// out_type: -1 x's type, 0 float32, 1 bfloat16
Tensor bn_relu_drop(const Tensor& x_in, const Tensor& gamma, const Tensor& beta, const Tensor& mov_mean, const Tensor& mov_var,
                    bool training, bool relu, unsigned long long thr, double scale, unsigned seed, double momentum, double eps,
                    int out_type) {
    TORCH_CHECK(x_in.defined() && (x_in.scalar_type() == at::kFloat || is_bf16(x_in)), "bn_relu_drop: x must be float32 or bfloat16");
    check_dev(x_in, x_in.scalar_type(), "x");
    TORCH_CHECK(out_type >= -1 && out_type <= 1, "bn_relu_drop: out_type must be -1 (x's type), 0 (float32) or 1 (bfloat16)");
    const bool x_bf16 = is_bf16(x_in), y_bf16 = out_type < 0 ? x_bf16 : out_type == 1;
    TORCH_CHECK(!(x_bf16 || y_bf16) || (x_in.dim() == 2 && x_in.size(1) % 2 == 0), "bn_relu_drop: bfloat16 rows need an even number of columns");
    const Tensor x = bf16_rows_aligned(x_in);
    TORCH_CHECK(x.dim() == 2 && x.size(0) >= 1 && x.size(1) >= 1 && x.size(0) < (1ll << 31) && x.size(1) < (1ll << 31),
                "bn_relu_drop expects x with dimensions (n, c), n, c >= 1");
    for (const Tensor* t : {&gamma, &beta, &mov_mean, &mov_var}) {
        check_dev(*t, at::kFloat, "per-column tensor");
        TORCH_CHECK(t->dim() == 1 && t->size(0) == x.size(1) && t->device() == x.device(), "bn_relu_drop: per-column tensors must have shape (c,)");
    }
    const DevGuard device_guard((int)x.device().index());
    const int n = (int)x.size(0), c = (int)x.size(1);
    const bool need_grad = at::GradMode::is_enabled() && (x_in.requires_grad() || gamma.requires_grad() || beta.requires_grad());
    TORCH_CHECK(training || !need_grad, "bn_relu_drop: the eval form has no gradients");
    Tensor y, saved;
    {
        at::AutoDispatchBelowADInplaceOrView guard;
        y = at::empty(x.sizes(), x.options().dtype(y_bf16 ? at::kBFloat16 : at::kFloat));
        if (training) saved = at::empty({2, (int64_t)c}, gamma.options());
        void* st = cur_stream(x);
        const size_t wsb = training ? mccnn_bn_act_workspace_bytes(n, c) : 0;
        Tensor& ws = scratch(wsb, x, st);
        check(mccnn_bn_act_fwd_rows(x.data_ptr(), x_bf16 ? 1 : 0, n, c, gamma.data_ptr<float>(), beta.data_ptr<float>(),
                                    mov_mean.data_ptr<float>(), mov_var.data_ptr<float>(), (float)momentum, (float)eps, training ? 1 : 0,
                                    relu ? 1 : 0, training ? thr : mccnn::kBnDropAll, training ? (float)scale : 1.f, seed, y.data_ptr(),
                                    y_bf16 ? 1 : 0, training ? saved.data_ptr<float>() : nullptr, ws.data_ptr(), (size_t)ws.numel(), st),
              "bn_relu_dropout");
    }
    if (need_grad) {
        auto node = std::shared_ptr<BnActBackward>(new BnActBackward(), torch::autograd::deleteNode);
        node->set_next_edges(torch::autograd::collect_next_edges(x_in, gamma, beta));
        node->x_ = x; node->gamma_ = gamma; node->beta_ = beta; node->y_bf16 = y_bf16;   // (x: the aligned copy where one was made)
        node->versions[0] = x._version(); node->versions[1] = gamma._version(); node->versions[2] = beta._version();
        node->saved = saved;
        node->relu = relu ? 1 : 0; node->thr = thr; node->scale = (float)scale; node->seed = seed;
        torch::autograd::set_history(y, node);
    }
    return y;
}

// ---- ... over a column-wise concatenation that is never materialised (mccnn_bn_act_cat_fwd_rows / _bwd_rows): the C++ form
// of dense_glue.bn_relu_dropout_cat -- the same library calls with the same arguments, so the same bytes. Every segment f32 or
// bf16 on its own, dx_s of x_s's type; a segment that does not require a gradient gets none (a NULL pointer in the call, an
// undefined tensor out of the node).
struct BnCatBackward : public torch::autograd::Node {
    std::vector<Tensor> xs;
    std::vector<uint32_t> x_versions;
    Tensor gamma_, beta_, saved;
    bool y_bf16 = false;
    uint32_t versions[2] = {0, 0};
    int relu = 1;
    unsigned long long thr = 0;
    float scale = 1.f;
    unsigned seed = 0;

    // inputs of the node: the segments in order, then gamma, then beta
    torch::autograd::variable_list apply(torch::autograd::variable_list&& grads) override {
        TORCH_CHECK(!xs.empty(), "bn_relu_drop_cat: backward through a graph whose buffers have been freed (retain_graph=True?)");
        const int nseg = (int)xs.size(), n = (int)xs[0].size(0), c = (int)gamma_.size(0);
        Tensor g0 = grads[0];   // (no tensor of y's shape is kept: zeros where autograd hands nothing over are made here)
        if (!g0.defined()) g0 = at::zeros({(int64_t)n, (int64_t)c}, gamma_.options().dtype(y_bf16 ? at::kBFloat16 : at::kFloat));
        const Tensor gy = bf16_rows_aligned(glue_grad_in("bn_relu_drop_cat", saved.defined(), g0, {&gamma_, &beta_}, versions, g0, y_bf16));
        for (int k = 0; k < nseg; ++k)
            TORCH_CHECK(xs[k]._version() == x_versions[k],
                        "one of the variables needed for gradient computation has been modified by an inplace operation (bn_relu_drop_cat "
                        "segment ", k, ")");
        const DevGuard device_guard((int)gamma_.device().index());
        std::vector<Tensor> dxs(nseg);
        const void* px[8];
        void* pdx[8];
        int cs[8], bf[8];
        bool any = false;
        for (int k = 0; k < nseg; ++k) {
            px[k] = xs[k].data_ptr();
            bf[k] = is_bf16(xs[k]) ? 1 : 0;
            cs[k] = (int)xs[k].size(1);
            pdx[k] = nullptr;
            if (task_should_compute_output(k)) {
                dxs[k] = at::empty_like(xs[k]);
                pdx[k] = dxs[k].data_ptr();
                any = true;
            }
        }
        Tensor dgb = at::empty({2, (int64_t)c}, gamma_.options());
        void* st = cur_stream(gamma_);
        Tensor& ws = scratch(mccnn_bn_act_workspace_bytes(n, c), gamma_, st);
        check(mccnn_bn_act_cat_bwd_rows(px, bf, cs, nseg, gy.data_ptr(), y_bf16 ? 1 : 0, n, gamma_.data_ptr<float>(),
                                        beta_.data_ptr<float>(), saved.data_ptr<float>(), relu, thr, scale, seed, any ? pdx : nullptr,
                                        dgb.data_ptr<float>(), dgb.data_ptr<float>() + c, ws.data_ptr(), (size_t)ws.numel(), st),
              "bn_relu_dropout_cat_grad");
        torch::autograd::variable_list out(nseg + 2);
        for (int k = 0; k < nseg; ++k) out[k] = dxs[k];
        if (task_should_compute_output(nseg)) out[nseg] = dgb.select(0, 0);
        if (task_should_compute_output(nseg + 1)) out[nseg + 1] = dgb.select(0, 1);
        return out;
    }
    void release_variables() override { xs.clear(); gamma_.reset(); beta_.reset(); saved.reset(); }
};

// out_type: 0 float32, 1 bfloat16, -1 what torch.cat of the segments has (bfloat16 iff every segment is). The caller (dense_glue._bn_cat_args) has checked the arguments; what is looked at
// here again is what this function itself relies on.
Tensor bn_relu_drop_cat(const std::vector<Tensor>& xs, const Tensor& gamma, const Tensor& beta, const Tensor& mov_mean,
                        const Tensor& mov_var, bool training, bool relu, unsigned long long thr, double scale, unsigned seed,
                        double momentum, double eps, int out_type) {
    TORCH_CHECK(!xs.empty() && (int)xs.size() <= mccnn_bn_act_cat_max_segments(), "bn_relu_drop_cat expects 1 to 8 segments");
    TORCH_CHECK(out_type >= -1 && out_type <= 1, "bn_relu_drop_cat: out_type must be -1 (the segments'), 0 (float32) or 1 (bfloat16)");
    bool all_bf16 = true;
    int64_t c64 = 0;
    bool need_grad = at::GradMode::is_enabled() && (gamma.requires_grad() || beta.requires_grad());
    for (const Tensor& x : xs) {
        check_dev(x, is_bf16(x) ? at::kBFloat16 : at::kFloat, "segment");
        all_bf16 = all_bf16 && is_bf16(x);
        TORCH_CHECK(x.dim() == 2 && x.size(0) >= 1 && x.size(1) >= 1 && x.size(0) == xs[0].size(0) && x.device() == xs[0].device(),
                    "bn_relu_drop_cat expects segments with dimensions (n, c_s) on one device, n, c_s >= 1");
        c64 += x.size(1);
        need_grad = need_grad || (at::GradMode::is_enabled() && x.requires_grad());
    }
    TORCH_CHECK(xs[0].size(0) < (1ll << 31) && c64 < (1ll << 31), "bn_relu_drop_cat: x too large");
    const bool y_bf16 = out_type == 1 || (out_type == -1 && all_bf16);
    TORCH_CHECK(!y_bf16 || c64 % 2 == 0, "bn_relu_drop_cat: bfloat16 rows need an even number of columns");
    for (const Tensor* t : {&gamma, &beta, &mov_mean, &mov_var}) {
        check_dev(*t, at::kFloat, "per-column tensor");
        TORCH_CHECK(t->dim() == 1 && t->size(0) == c64 && t->device() == xs[0].device(), "bn_relu_drop_cat: per-column tensors must have shape (C,)");
    }
    TORCH_CHECK(training || !need_grad, "bn_relu_drop_cat: the eval form has no gradients");
    const DevGuard device_guard((int)gamma.device().index());
    const int nseg = (int)xs.size(), n = (int)xs[0].size(0), c = (int)c64;
    Tensor y, saved;
    {
        at::AutoDispatchBelowADInplaceOrView guard;
        y = at::empty({(int64_t)n, c64}, gamma.options().dtype(y_bf16 ? at::kBFloat16 : at::kFloat));
        if (training) saved = at::empty({2, c64}, gamma.options());
        const void* px[8];
        int cs[8], bf[8];
        for (int k = 0; k < nseg; ++k) { px[k] = xs[k].data_ptr(); bf[k] = is_bf16(xs[k]) ? 1 : 0; cs[k] = (int)xs[k].size(1); }
        void* st = cur_stream(gamma);
        Tensor& ws = scratch(training ? mccnn_bn_act_workspace_bytes(n, c) : 0, gamma, st);
        check(mccnn_bn_act_cat_fwd_rows(px, bf, cs, nseg, n, gamma.data_ptr<float>(), beta.data_ptr<float>(), mov_mean.data_ptr<float>(),
                                        mov_var.data_ptr<float>(), (float)momentum, (float)eps, training ? 1 : 0, relu ? 1 : 0,
                                        training ? thr : mccnn::kBnDropAll, training ? (float)scale : 1.f, seed, y.data_ptr(),
                                        y_bf16 ? 1 : 0, training ? saved.data_ptr<float>() : nullptr, ws.data_ptr(), (size_t)ws.numel(), st),
              "bn_relu_dropout_cat");
    }
    if (need_grad) {
        auto node = std::shared_ptr<BnCatBackward>(new BnCatBackward(), torch::autograd::deleteNode);
        node->set_next_edges(torch::autograd::collect_next_edges(xs, gamma, beta));
        for (const Tensor& x : xs) { node->xs.push_back(x.detach()); node->x_versions.push_back(x._version()); }
        node->gamma_ = gamma; node->beta_ = beta; node->y_bf16 = y_bf16;
        node->versions[0] = gamma._version(); node->versions[1] = beta._version();
        node->saved = saved;
        node->relu = relu ? 1 : 0; node->thr = thr; node->scale = (float)scale; node->seed = seed;
        torch::autograd::set_history(y, node);
    }
    return y;
}

// ---- ... with batch statistics across ranks (mccnn_bn_sync_*): the four stages as they are. The collectives between them
// are torch.distributed's, so the autograd node is Python's (dense_glue._BnReluDropoutSync), which has checked the
// arguments; here only what keeps a call inside its tensors. x / dx and y / dy are each f32 or bf16 rows.
struct BnSyncShape {
    int n, c, x_bf16;
};
BnSyncShape bn_sync_shape(const Tensor& x, int64_t rank, int64_t world, const Tensor& parts) {
    TORCH_CHECK(x.defined() && (x.scalar_type() == at::kFloat || is_bf16(x)), "bn_relu_drop_sync: x must be float32 or bfloat16");
    check_dev(x, x.scalar_type(), "x");
    TORCH_CHECK(x.dim() == 2 && x.size(0) >= 1 && x.size(1) >= 1 && x.size(0) < (1ll << 31) && x.size(1) < (1ll << 31),
                "bn_relu_drop_sync expects x with dimensions (n, c), n, c >= 1");
    TORCH_CHECK(world >= 1 && rank >= 0 && rank < world, "bn_relu_drop_sync: rank outside [0, world)");
    check_dev(parts, at::kFloat, "rank partials");
    TORCH_CHECK(parts.numel() == world * 3 * x.size(1) && parts.device() == x.device(), "bn_relu_drop_sync: the rank partials must be [world, 3, c]");
    return {(int)x.size(0), (int)x.size(1), is_bf16(x) ? 1 : 0};
}
void bn_sync_cols(const Tensor& x, int64_t rows, std::initializer_list<const Tensor*> ts) {
    for (const Tensor* t : ts) {
        check_dev(*t, at::kFloat, "per-column tensor");
        TORCH_CHECK(t->numel() == rows * x.size(1) && t->device() == x.device(), "bn_relu_drop_sync: per-column tensors must have shape (c,)");
    }
}
void bn_sync_rows(const Tensor& x, const Tensor& t, const char* name) {
    TORCH_CHECK(t.defined() && (t.scalar_type() == at::kFloat || is_bf16(t)), "bn_relu_drop_sync: ", name, " must be float32 or bfloat16");
    check_dev(t, t.scalar_type(), name);
    TORCH_CHECK(t.sizes() == x.sizes() && t.device() == x.device(), "bn_relu_drop_sync: ", name, " must have x's shape");
}
void bn_sync_meta(const Tensor& x, const Tensor& meta) {
    check_dev(meta, at::kInt, "meta");
    TORCH_CHECK(meta.numel() == 2 && meta.device() == x.device(), "bn_relu_drop_sync: meta must be int32 [2]");
}

void bn_sync_stats(const Tensor& x, int64_t rank, int64_t world, const Tensor& parts) {
    const BnSyncShape s = bn_sync_shape(x, rank, world, parts);
    const DevGuard device_guard((int)x.device().index());
    void* st = cur_stream(x);
    Tensor& ws = scratch(mccnn_bn_act_workspace_bytes(s.n, s.c), x, st);
    check(mccnn_bn_sync_stats(x.data_ptr(), s.x_bf16, s.n, s.c, (int)rank, (int)world, parts.data_ptr<float>(), ws.data_ptr(),
                              (size_t)ws.numel(), st),
          "bn_relu_dropout_sync");
}

void bn_sync_apply(const Tensor& x, int64_t rank, int64_t world, const Tensor& parts, const Tensor& gamma, const Tensor& beta,
                   const Tensor& mov_mean, const Tensor& mov_var, double momentum, double eps, bool relu, unsigned long long thr,
                   double scale, unsigned seed, const Tensor& y, const Tensor& saved, const Tensor& meta) {
    const BnSyncShape s = bn_sync_shape(x, rank, world, parts);
    bn_sync_cols(x, 1, {&gamma, &beta, &mov_mean, &mov_var});
    bn_sync_cols(x, 2, {&saved});
    bn_sync_rows(x, y, "y");
    bn_sync_meta(x, meta);
    const DevGuard device_guard((int)x.device().index());
    check(mccnn_bn_sync_apply(x.data_ptr(), s.x_bf16, s.n, s.c, (int)rank, (int)world, parts.data_ptr<float>(), gamma.data_ptr<float>(),
                              beta.data_ptr<float>(), mov_mean.data_ptr<float>(), mov_var.data_ptr<float>(), (float)momentum,
                              (float)eps, relu ? 1 : 0, thr, (float)scale, seed, y.data_ptr(), is_bf16(y) ? 1 : 0,
                              saved.data_ptr<float>(), meta.data_ptr<int>(), cur_stream(x)),
          "bn_relu_dropout_sync");
}

void bn_sync_bwd_sums(const Tensor& x, const Tensor& dy, int64_t rank, int64_t world, const Tensor& gamma, const Tensor& beta,
                      const Tensor& saved, const Tensor& meta, bool relu, unsigned long long thr, double scale, unsigned seed,
                      const Tensor& parts_b, const Tensor& dgb) {
    const BnSyncShape s = bn_sync_shape(x, rank, world, parts_b);
    bn_sync_cols(x, 1, {&gamma, &beta});
    bn_sync_cols(x, 2, {&saved, &dgb});
    bn_sync_rows(x, dy, "dy");
    bn_sync_meta(x, meta);
    const DevGuard device_guard((int)x.device().index());
    void* st = cur_stream(x);
    Tensor& ws = scratch(mccnn_bn_act_workspace_bytes(s.n, s.c), x, st);
    check(mccnn_bn_sync_bwd_sums(x.data_ptr(), s.x_bf16, dy.data_ptr(), is_bf16(dy) ? 1 : 0, s.n, s.c, (int)rank, (int)world,
                                 gamma.data_ptr<float>(), beta.data_ptr<float>(), saved.data_ptr<float>(), meta.data_ptr<int>(),
                                 relu ? 1 : 0, thr, (float)scale, seed, parts_b.data_ptr<float>(), dgb.data_ptr<float>(),
                                 dgb.data_ptr<float>() + s.c, ws.data_ptr(), (size_t)ws.numel(), st),
          "bn_relu_dropout_sync_grad");
}

// dgb: the [2, c] (dgamma; dbeta) of bn_sync_bwd_sums, whose first row is completed here
void bn_sync_bwd_dx(const Tensor& x, const Tensor& dy, int64_t rank, int64_t world, const Tensor& gamma, const Tensor& beta,
                    const Tensor& parts_b, const Tensor& saved, const Tensor& meta, bool relu, unsigned long long thr, double scale,
                    unsigned seed, const c10::optional<Tensor>& dx, const Tensor& dgb) {
    const BnSyncShape s = bn_sync_shape(x, rank, world, parts_b);
    bn_sync_cols(x, 1, {&gamma, &beta});
    bn_sync_cols(x, 2, {&saved, &dgb});
    bn_sync_rows(x, dy, "dy");
    bn_sync_meta(x, meta);
    const bool want_dx = dx.has_value() && dx->defined();
    if (want_dx) {
        bn_sync_rows(x, *dx, "dx");
        TORCH_CHECK(dx->scalar_type() == x.scalar_type(), "bn_relu_drop_sync: dx must have x's type");
    }
    const DevGuard device_guard((int)x.device().index());
    check(mccnn_bn_sync_bwd_dx(x.data_ptr(), s.x_bf16, dy.data_ptr(), is_bf16(dy) ? 1 : 0, s.n, s.c, (int)rank, (int)world,
                               gamma.data_ptr<float>(), beta.data_ptr<float>(), parts_b.data_ptr<float>(), saved.data_ptr<float>(),
                               meta.data_ptr<int>(), relu ? 1 : 0, thr, (float)scale, seed, want_dx ? dx->data_ptr() : nullptr,
                               dgb.data_ptr<float>(), cur_stream(x)),
          "bn_relu_dropout_sync_grad");
}

// ---- a linear layer and the dense glue behind it as one op (mccnn_linear_bn_act_fwd / _bwd): y = drop(act(bn(x w + b))), the
// C++ form of dense_glue.linear_bn_relu_dropout -- the same library calls with the same arguments, so the same bytes.
// x, w, z and everything per column are f32; y (and dy) f32 or bf16.
struct LinearBnBackward : public torch::autograd::Node {
    Tensor x_, w_, gamma_, beta_, z, saved;
    bool y_bf16 = false;
    uint32_t versions[4] = {0, 0, 0, 0};
    int relu = 1;
    unsigned long long thr = 0;
    float scale = 1.f;
    unsigned seed = 0;

    torch::autograd::variable_list apply(torch::autograd::variable_list&& grads) override {
        const Tensor gy = glue_grad_in("linear_bn_relu_drop", x_.defined() && z.defined() && saved.defined(), grads[0],
                                       {&x_, &w_, &gamma_, &beta_}, versions, z, y_bf16);
        const DevGuard device_guard((int)x_.device().index());
        const int n = (int)x_.size(0), cin = (int)x_.size(1), cout = (int)w_.size(1);
        const bool want_dx = task_should_compute_output(0);
        Tensor dx;
        if (want_dx) dx = at::empty_like(x_);
        Tensor dw = at::empty_like(w_);
        Tensor dv = at::empty({3, (int64_t)cout}, gamma_.options());   // db, dgamma, dbeta
        void* st = cur_stream(x_);
        Tensor& ws = scratch(mccnn_linear_bn_act_workspace_bytes(n, cin, cout), x_, st);
        check(mccnn_linear_bn_act_bwd(x_.data_ptr<float>(), w_.data_ptr<float>(), z.data_ptr<float>(), gy.data_ptr(), y_bf16 ? 1 : 0, n,
                                      cin, cout, gamma_.data_ptr<float>(), beta_.data_ptr<float>(), saved.data_ptr<float>(), relu, thr,
                                      scale, seed, want_dx ? dx.data_ptr<float>() : nullptr, dw.data_ptr<float>(), dv.data_ptr<float>(),
                                      dv.data_ptr<float>() + cout, dv.data_ptr<float>() + 2 * (size_t)cout, ws.data_ptr(),
                                      (size_t)ws.numel(), st),
              "linear_bn_relu_dropout_grad");
        torch::autograd::variable_list out(5);
        out[0] = dx;
        if (task_should_compute_output(1)) out[1] = dw;
        if (task_should_compute_output(2)) out[2] = dv.select(0, 0);
        if (task_should_compute_output(3)) out[3] = dv.select(0, 1);
        if (task_should_compute_output(4)) out[4] = dv.select(0, 2);
        return out;
    }
    void release_variables() override { x_.reset(); w_.reset(); gamma_.reset(); beta_.reset(); z.reset(); saved.reset(); }
};

// out_type: -1 or 0 float32, 1 bfloat16
Tensor linear_bn_relu_drop(const Tensor& x, const Tensor& w, const Tensor& b, const Tensor& gamma, const Tensor& beta,
                           const Tensor& mov_mean, const Tensor& mov_var, bool training, bool relu, unsigned long long thr,
                           double scale, unsigned seed, double momentum, double eps, int out_type) {
    check_dev(x, at::kFloat, "x");
    check_dev(w, at::kFloat, "w");
    TORCH_CHECK(out_type >= -1 && out_type <= 1, "linear_bn_relu_drop: out_type must be -1 / 0 (float32) or 1 (bfloat16)");
    const bool y_bf16 = out_type == 1;
    TORCH_CHECK(x.dim() == 2 && w.dim() == 2 && x.size(0) >= 1 && x.size(1) >= 1 && w.size(1) >= 1 && w.size(0) == x.size(1) &&
                    x.size(0) < (1ll << 31) && x.size(1) < (1ll << 31) && w.size(1) < (1ll << 31) && w.device() == x.device(),
                "linear_bn_relu_drop expects x (n, cin) and w (cin, cout), n, cin, cout >= 1");
    TORCH_CHECK(!y_bf16 || w.size(1) % 2 == 0, "linear_bn_relu_drop: bfloat16 rows need an even number of columns");
    for (const Tensor* t : {&b, &gamma, &beta, &mov_mean, &mov_var}) {
        check_dev(*t, at::kFloat, "per-column tensor");
        TORCH_CHECK(t->dim() == 1 && t->size(0) == w.size(1) && t->device() == x.device(),
                    "linear_bn_relu_drop: per-column tensors must have shape (cout,)");
    }
    const DevGuard device_guard((int)x.device().index());
    const int n = (int)x.size(0), cin = (int)x.size(1), cout = (int)w.size(1);
    const bool need_grad = at::GradMode::is_enabled() &&
                           (x.requires_grad() || w.requires_grad() || b.requires_grad() || gamma.requires_grad() || beta.requires_grad());
    TORCH_CHECK(training || !need_grad, "linear_bn_relu_drop: the eval form has no gradients");
    Tensor y, z, saved;
    {
        at::AutoDispatchBelowADInplaceOrView guard;
        y = at::empty({(int64_t)n, (int64_t)cout}, x.options().dtype(y_bf16 ? at::kBFloat16 : at::kFloat));
        if (training) {
            z = at::empty({(int64_t)n, (int64_t)cout}, x.options());
            saved = at::empty({3, (int64_t)cout}, gamma.options());
        }
        void* st = cur_stream(x);
        Tensor& ws = scratch(training ? mccnn_linear_bn_act_workspace_bytes(n, cin, cout) : 0, x, st);
        check(mccnn_linear_bn_act_fwd(x.data_ptr<float>(), w.data_ptr<float>(), b.data_ptr<float>(), n, cin, cout, gamma.data_ptr<float>(),
                                      beta.data_ptr<float>(), mov_mean.data_ptr<float>(), mov_var.data_ptr<float>(), (float)momentum,
                                      (float)eps, training ? 1 : 0, relu ? 1 : 0, training ? thr : mccnn::kBnDropAll,
                                      training ? (float)scale : 1.f, seed, training ? z.data_ptr<float>() : nullptr, y.data_ptr(),
                                      y_bf16 ? 1 : 0, training ? saved.data_ptr<float>() : nullptr, training ? ws.data_ptr() : nullptr,
                                      training ? (size_t)ws.numel() : 0, st),
              "linear_bn_relu_dropout");
    }
    if (need_grad) {
        auto node = std::shared_ptr<LinearBnBackward>(new LinearBnBackward(), torch::autograd::deleteNode);
        node->set_next_edges(torch::autograd::collect_next_edges(x, w, b, gamma, beta));
        node->x_ = x; node->w_ = w; node->gamma_ = gamma; node->beta_ = beta; node->y_bf16 = y_bf16;
        node->versions[0] = x._version(); node->versions[1] = w._version(); node->versions[2] = gamma._version();
        node->versions[3] = beta._version();
        node->z = z; node->saved = saved;
        node->relu = relu ? 1 : 0; node->thr = thr; node->scale = (float)scale; node->seed = seed;
        torch::autograd::set_history(y, node);
    }
    return y;
}

// ---- the last linear layer and the softmax cross-entropy behind it as one op (mccnn_linear_xent_fwd / _bwd), the C++ form of
// dense_glue.linear_softmax_xent -- the same library calls with the same arguments, so the same bytes. Python has checked the
// arguments (labels int32 [n], weights f32 [n] or None); here only what keeps a call inside its tensors. loss alone carries
// the node: pred, meta and the logits have no history.
struct LinearXentBackward : public torch::autograd::Node {
    Tensor x_, w_, b_, labels, rw, lse, meta;
    uint32_t versions[3] = {0, 0, 0};

    torch::autograd::variable_list apply(torch::autograd::variable_list&& grads) override {
        const Tensor g = glue_grad_in("linear_softmax_xent", x_.defined() && lse.defined() && meta.defined(), grads[0], {&x_, &w_, &b_},
                                      versions, lse.select(0, 0), false);
        TORCH_CHECK(g.numel() == 1 && g.is_cuda() && g.device() == x_.device(), "linear_softmax_xent: the gradient of loss must be one word on x's device");
        const DevGuard device_guard((int)x_.device().index());
        const int n = (int)x_.size(0), cin = (int)x_.size(1), c = (int)w_.size(1);
        const bool want_dx = task_should_compute_output(0);
        Tensor dx;
        if (want_dx) dx = at::empty_like(x_);
        Tensor dw = at::empty_like(w_);
        Tensor db = at::empty_like(b_);
        void* st = cur_stream(x_);
        Tensor& ws = scratch(mccnn_linear_xent_workspace_bytes(n, cin, c), x_, st);
        check(mccnn_linear_xent_bwd(x_.data_ptr<float>(), w_.data_ptr<float>(), b_.data_ptr<float>(), n, cin, c, labels.data_ptr<int>(),
                                    rw.defined() ? rw.data_ptr<float>() : nullptr, lse.data_ptr<float>(), meta.data_ptr<int>(),
                                    g.data_ptr<float>(), want_dx ? dx.data_ptr<float>() : nullptr, dw.data_ptr<float>(),
                                    db.data_ptr<float>(), ws.data_ptr(), (size_t)ws.numel(), st),
              "linear_softmax_xent_grad");
        torch::autograd::variable_list out(3);
        out[0] = dx;
        if (task_should_compute_output(1)) out[1] = dw;
        if (task_should_compute_output(2)) out[2] = db;
        return out;
    }
    void release_variables() override { x_.reset(); w_.reset(); b_.reset(); labels.reset(); rw.reset(); lse.reset(); meta.reset(); }
};

// -> (loss [], pred [n] int32, meta [2] int32 = D, correct, logits [n, c] or an undefined tensor)
std::tuple<Tensor, Tensor, Tensor, Tensor> linear_softmax_xent(const Tensor& x, const Tensor& w, const Tensor& b, const Tensor& labels,
                                                               const c10::optional<Tensor>& weights, bool want_logits) {
    check_dev(x, at::kFloat, "x");
    check_dev(w, at::kFloat, "w");
    check_dev(b, at::kFloat, "b");
    check_dev(labels, at::kInt, "labels");
    TORCH_CHECK(x.dim() == 2 && w.dim() == 2 && x.size(0) >= 1 && x.size(1) >= 1 && w.size(1) >= 1 && w.size(0) == x.size(1) &&
                    x.size(0) < (1ll << 31) && x.size(1) < (1ll << 31) && w.size(1) < (1ll << 31) && w.device() == x.device(),
                "linear_softmax_xent expects x (n, cin) and w (cin, c), n, cin, c >= 1");
    TORCH_CHECK(b.dim() == 1 && b.size(0) == w.size(1) && b.device() == x.device(), "linear_softmax_xent: b must have shape (c,)");
    TORCH_CHECK(labels.numel() == x.size(0) && labels.device() == x.device(), "linear_softmax_xent: labels must have n elements");
    Tensor rw;
    if (weights.has_value() && weights->defined()) {
        rw = *weights;
        check_dev(rw, at::kFloat, "weights");
        TORCH_CHECK(rw.numel() == x.size(0) && rw.device() == x.device(), "linear_softmax_xent: weights must have n elements");
    }
    const DevGuard device_guard((int)x.device().index());
    const int n = (int)x.size(0), cin = (int)x.size(1), c = (int)w.size(1);
    const bool need_grad = at::GradMode::is_enabled() && (x.requires_grad() || w.requires_grad() || b.requires_grad());
    Tensor loss, lse, pred, meta, logits;
    {
        at::AutoDispatchBelowADInplaceOrView guard;
        loss = at::empty({}, x.options());
        lse = at::empty({(int64_t)n}, x.options());
        pred = at::empty({(int64_t)n}, labels.options());
        meta = at::empty({2}, labels.options());
        if (want_logits) logits = at::empty({(int64_t)n, (int64_t)c}, x.options());
        void* st = cur_stream(x);
        Tensor& ws = scratch(mccnn_linear_xent_workspace_bytes(n, cin, c), x, st);
        check(mccnn_linear_xent_fwd(x.data_ptr<float>(), w.data_ptr<float>(), b.data_ptr<float>(), n, cin, c, labels.data_ptr<int>(),
                                    rw.defined() ? rw.data_ptr<float>() : nullptr, loss.data_ptr<float>(), lse.data_ptr<float>(),
                                    meta.data_ptr<int>(), pred.data_ptr<int>(), want_logits ? logits.data_ptr<float>() : nullptr,
                                    ws.data_ptr(), (size_t)ws.numel(), st),
              "linear_softmax_xent");
    }
    if (need_grad) {
        auto node = std::shared_ptr<LinearXentBackward>(new LinearXentBackward(), torch::autograd::deleteNode);
        node->set_next_edges(torch::autograd::collect_next_edges(x, w, b));
        node->x_ = x; node->w_ = w; node->b_ = b; node->labels = labels; node->rw = rw; node->lse = lse; node->meta = meta;
        node->versions[0] = x._version(); node->versions[1] = w._version(); node->versions[2] = b._version();
        torch::autograd::set_history(loss, node);
    }
    return std::make_tuple(loss, pred, meta, logits);
}

// ---- the cosine-distance loss of normal estimation as one op (mccnn_cosine_loss_fwd / _bwd), the C++ form of
// dense_glue.cosine_distance_loss -- the same library calls with the same arguments, so the same bytes. Python has checked the
// arguments (weights f32 [n] or None, no gradient asked of target or weights); here only what keeps a call inside its tensors.
// loss alone carries the node: sums and meta have no history.
struct CosineLossBackward : public torch::autograd::Node {
    Tensor pred_, target_, rw, sums, meta;
    uint32_t versions[2] = {0, 0};

    torch::autograd::variable_list apply(torch::autograd::variable_list&& grads) override {
        const Tensor g = glue_grad_in("cosine_distance_loss", pred_.defined() && sums.defined() && meta.defined(), grads[0],
                                      {&pred_, &target_}, versions, sums.select(0, 0), false);
        TORCH_CHECK(g.numel() == 1 && g.is_cuda() && g.device() == pred_.device(),
                    "cosine_distance_loss: the gradient of loss must be one word on pred's device");
        const DevGuard device_guard((int)pred_.device().index());
        const int n = (int)pred_.size(0), c = (int)pred_.size(1);
        Tensor dp = at::empty_like(pred_);
        check(mccnn_cosine_loss_bwd(pred_.data_ptr<float>(), target_.data_ptr<float>(), n, c, rw.defined() ? rw.data_ptr<float>() : nullptr,
                                    meta.data_ptr<int>(), g.data_ptr<float>(), dp.data_ptr<float>(), cur_stream(pred_)),
              "cosine_distance_loss_grad");
        torch::autograd::variable_list out(1);
        out[0] = dp;
        return out;
    }
    void release_variables() override { pred_.reset(); target_.reset(); rw.reset(); sums.reset(); meta.reset(); }
};

// -> (loss [], sums [2] = cosSum, angleSum, meta [1] int32 = D)
std::tuple<Tensor, Tensor, Tensor> cosine_distance_loss(const Tensor& pred, const Tensor& target, const c10::optional<Tensor>& weights) {
    check_dev(pred, at::kFloat, "pred");
    check_dev(target, at::kFloat, "target");
    TORCH_CHECK(pred.dim() == 2 && pred.size(0) >= 1 && pred.size(1) >= 1 && pred.size(0) * pred.size(1) < (1ll << 31) &&
                    target.sizes() == pred.sizes() && target.device() == pred.device(),
                "cosine_distance_loss expects pred (n, c) and target (n, c), n, c >= 1");
    Tensor rw;
    if (weights.has_value() && weights->defined()) {
        rw = *weights;
        check_dev(rw, at::kFloat, "weights");
        TORCH_CHECK(rw.numel() == pred.size(0) && rw.device() == pred.device(), "cosine_distance_loss: weights must have n elements");
    }
    const DevGuard device_guard((int)pred.device().index());
    const int n = (int)pred.size(0), c = (int)pred.size(1);
    const bool need_grad = at::GradMode::is_enabled() && pred.requires_grad();
    Tensor loss, sums, meta;
    {
        at::AutoDispatchBelowADInplaceOrView guard;
        loss = at::empty({}, pred.options());
        sums = at::empty({2}, pred.options());
        meta = at::empty({1}, pred.options().dtype(at::kInt));
        void* st = cur_stream(pred);
        Tensor& ws = scratch(mccnn_cosine_loss_workspace_bytes(n, c), pred, st);
        check(mccnn_cosine_loss_fwd(pred.data_ptr<float>(), target.data_ptr<float>(), n, c, rw.defined() ? rw.data_ptr<float>() : nullptr,
                                    loss.data_ptr<float>(), sums.data_ptr<float>(), meta.data_ptr<int>(), ws.data_ptr(),
                                    (size_t)ws.numel(), st),
              "cosine_distance_loss");
    }
    if (need_grad) {
        auto node = std::shared_ptr<CosineLossBackward>(new CosineLossBackward(), torch::autograd::deleteNode);
        node->set_next_edges(torch::autograd::collect_next_edges(pred));
        node->pred_ = pred; node->target_ = target; node->rw = rw; node->sums = sums; node->meta = meta;
        node->versions[0] = pred._version(); node->versions[1] = target._version();
        torch::autograd::set_history(loss, node);
    }
    return std::make_tuple(loss, sums, meta);
}

// ---- segmentation scores on the device: per-cloud, per-class counts (mccnn_seg_counts_add), the C++ form of
// dense_glue.segmentation_counts -- the same library call with the same arguments, so the same bytes. Python has checked the
// arguments and cast int64 pred / labels; here only what keeps the call inside its tensors. A plain function on the current
// stream: nothing is differentiable. -> counts int64 [num_clouds, num_classes, 3] (out, added to, when given; else zeroed)
Tensor segmentation_counts(const Tensor& pred, const Tensor& labels, int64_t num_classes, const c10::optional<Tensor>& batch_ids,
                           int64_t num_clouds, const c10::optional<Tensor>& weights, int64_t ignore_label,
                           const c10::optional<Tensor>& out) {
    check_dev(pred, at::kInt, "pred");
    check_dev(labels, at::kInt, "labels");
    const int64_t n = pred.numel();
    TORCH_CHECK(num_classes >= 1 && num_clouds >= 1 && num_clouds * num_classes * 3 < (1ll << 31) && n < (1ll << 31) &&
                    labels.numel() == n && labels.device() == pred.device() && ignore_label >= -1 && ignore_label < (1ll << 31),
                "segmentation_counts expects pred (n,) and labels (n,) int32, numClouds, numClasses >= 1");
    Tensor bi, rw, counts;
    if (batch_ids.has_value() && batch_ids->defined()) {
        bi = *batch_ids;
        check_dev(bi, at::kInt, "batchIds");
        TORCH_CHECK(bi.numel() == n && bi.device() == pred.device(), "segmentation_counts: batchIds must have n elements");
    }
    if (weights.has_value() && weights->defined()) {
        rw = *weights;
        check_dev(rw, at::kFloat, "weights");
        TORCH_CHECK(rw.numel() == n && rw.device() == pred.device(), "segmentation_counts: weights must have n elements");
    }
    const DevGuard device_guard((int)pred.device().index());
    if (out.has_value() && out->defined()) {
        counts = *out;
        check_dev(counts, at::kLong, "out");
        TORCH_CHECK(counts.dim() == 3 && counts.size(0) == num_clouds && counts.size(1) == num_classes && counts.size(2) == 3 &&
                        counts.device() == pred.device(),
                    "segmentation_counts: out must have shape (numClouds, numClasses, 3)");
    } else {
        counts = at::zeros({num_clouds, num_classes, 3}, pred.options().dtype(at::kLong));
    }
    check(mccnn_seg_counts_add(pred.data_ptr<int>(), labels.data_ptr<int>(), rw.defined() ? rw.data_ptr<float>() : nullptr,
                               bi.defined() ? bi.data_ptr<int>() : nullptr, (int)n, (int)num_clouds, (int)num_classes,
                               (int)ignore_label, reinterpret_cast<long long*>(counts.data_ptr<int64_t>()), cur_stream(pred)),
          "segmentation_counts");
    return counts;
}

// ---- voxel accuracy on the device: per-voxel majority votes (mccnn_voxel_acc_add), the C++ form of dense_glue.voxel_counts
// -- the same library call with the same arguments and the same table (ws: Python's zeroed tensor, handed over clean and left
// clean), so the same bytes. Python has checked the arguments and cast int64 pred / labels; here only what keeps the call
// inside its tensors. -> counts int64 [num_clouds, num_classes, 2] (out, added to, when given; else zeroed)
Tensor voxel_counts(const Tensor& points, const Tensor& pred, const Tensor& labels, int64_t num_classes,
                    const c10::optional<Tensor>& batch_ids, int64_t num_clouds, const Tensor& aabb_min, double resolution,
                    int64_t ignore_label, double max_ignore_share, const c10::optional<Tensor>& out,
                    const c10::optional<Tensor>& dropped, const c10::optional<Tensor>& ws) {
    check_dev(points, at::kFloat, "points");
    check_dev(pred, at::kInt, "pred");
    check_dev(labels, at::kInt, "labels");
    check_dev(aabb_min, at::kFloat, "aabbMin");
    TORCH_CHECK(points.dim() == 2 && points.size(1) == 3, "voxel_counts expects points (n, 3)");
    const int64_t n = points.size(0);
    TORCH_CHECK(num_classes >= 1 && num_clouds >= 1 && num_clouds <= 32768 && num_clouds * num_classes * 2 < (1ll << 31) &&
                    n < (1ll << 30) && pred.numel() == n && labels.numel() == n && aabb_min.numel() == num_clouds * 3 &&
                    pred.device() == points.device() && labels.device() == points.device() && aabb_min.device() == points.device() &&
                    ignore_label >= -1 && ignore_label < (1ll << 31),
                "voxel_counts expects points (n, 3) float32, pred (n,) and labels (n,) int32, aabbMin (numClouds, 3)");
    Tensor bi, counts, dr, table;
    if (batch_ids.has_value() && batch_ids->defined()) {
        bi = *batch_ids;
        check_dev(bi, at::kInt, "batchIds");
        TORCH_CHECK(bi.numel() == n && bi.device() == points.device(), "voxel_counts: batchIds must have n elements");
    }
    if (dropped.has_value() && dropped->defined()) {
        dr = *dropped;
        check_dev(dr, at::kInt, "dropped");
        TORCH_CHECK(dr.numel() == 1 && dr.device() == points.device(), "voxel_counts: dropped must have one element");
    }
    const DevGuard device_guard((int)points.device().index());
    if (out.has_value() && out->defined()) {
        counts = *out;
        check_dev(counts, at::kLong, "out");
        TORCH_CHECK(counts.dim() == 3 && counts.size(0) == num_clouds && counts.size(1) == num_classes && counts.size(2) == 2 &&
                        counts.device() == points.device(),
                    "voxel_counts: out must have shape (numClouds, numClasses, 2)");
    } else {
        counts = at::zeros({num_clouds, num_classes, 2}, points.options().dtype(at::kLong));
    }
    if (n == 0) return counts;
    TORCH_CHECK(ws.has_value() && ws->defined(), "voxel_counts: no table");
    table = *ws;
    check_dev(table, at::kByte, "ws");
    TORCH_CHECK(table.device() == points.device(), "voxel_counts: the table must be on points' device");
    check(mccnn_voxel_acc_add(points.data_ptr<float>(), pred.data_ptr<int>(), labels.data_ptr<int>(),
                              bi.defined() ? bi.data_ptr<int>() : nullptr, aabb_min.data_ptr<float>(), (int)n, (int)num_clouds,
                              (int)num_classes, (int)ignore_label, (float)resolution, max_ignore_share,
                              reinterpret_cast<long long*>(counts.data_ptr<int64_t>()), dr.defined() ? dr.data_ptr<int>() : nullptr,
                              table.data_ptr(), (size_t)table.numel(), 1, cur_stream(points)),
          "voxel_counts");
    return counts;
}

// ---- point hierarchy of the NEXT batch, built on a stream of its own by a helper thread -------------------------------
// A hierarchy depends on the points only. Built inline it is a chain of ~13 small dependent kernels per level that ends in
// a read-back of the level sizes (and, for an absolute radius, starts with one of the box extent): the host cannot issue
// anything of the step while it waits, and the GPU has nothing else to run. Requested one step ahead the chain runs under
// the convolutions of the batch in flight, and the calling thread never waits for the device.
// Memory: everything the caller will read (boxes, level rows) is allocated HERE, on the calling thread and its current
// stream, sized by the capacity (level 0's point count) -- the helper's stream starts behind an event recorded on the
// caller's stream at this moment, and the caller's stream joins the helper's event before the first use, so the blocks
// go back to the allocator they came from after every reader. Temporaries (sorted copies, cell tables, scan words) live
// in the helper thread's own scratch.
hipStream_t hier_stream() {
    static hipStream_t streams[kMaxDevices] = {};
    static bool made[kMaxDevices] = {};
    static std::mutex m;
    const int d = device_now();
    std::lock_guard<std::mutex> lk(m);
    if (!made[d]) {
        if (hipStreamCreateWithFlags(&streams[d], hipStreamNonBlocking) != hipSuccess) streams[d] = nullptr;
        made[d] = true;
    }
    return streams[d];
}

struct HierFuture {
    Tensor pts, bids, mn, mx, sizes;
    Tensor block;                    // prefetched hierarchies: the ONE allocation mn .. lfeats are views of
    std::vector<Tensor> ints, flts;  // per level: sampled batch ids | sampled indexs | transformed indexs   and   sampled points
    // optional: the input feature rows of level 0 (no gradient, short rows) -- every level's rows are then gathered HERE,
    // on the hierarchy's stream, once the level sizes are known (GetSampledFeatures, MCConvBuilder.py:112-116), instead
    // of by one launch per level on the calling thread when the hierarchy is adopted
    Tensor feats;
    std::vector<Tensor> lfeats;      // per level: [ca x F] rows
    std::vector<double> radii;
    std::vector<int> ncs, hs;
    int B = 0, L = 0, cap = 0, pmode = 1;
    int64_t ca = 0;
    bool scale_inv = true;
    float extent = 0.f;
    std::atomic<int> done{1};
    int rc = 0;
    std::string what;
    hipEvent_t event = nullptr;
    void* alloc_stream = nullptr;
    bool joined = false;

    void wait_done() {
        int spins = 0;
        while (!done.load(std::memory_order_acquire)) {
            if (++spins < 2000) continue;
            if (spins < 4000) std::this_thread::yield();
            else std::this_thread::sleep_for(std::chrono::microseconds(20));
        }
    }
    ~HierFuture() {
        wait_done();
        if (event) {
            if (!joined && rc == 0) (void)hipStreamWaitEvent((hipStream_t)alloc_stream, event, 0);
            give_event(event);
        }
    }

    // the helper thread's part: boxes, cell counts, the levels, ONE read-back of the sizes
    void run(hipStream_t ss) {
        try {
            enter_device((int)pts.device().index());
            const float* P = pts.data_ptr<float>();
            const int* Bi = bids.data_ptr<int>();
            float* pmn = mn.data_ptr<float>();
            float* pmx = mx.data_ptr<float>();
            const size_t aw = mccnn_compute_aabb_workspace_bytes(B);
            check(mccnn_compute_aabb(P, Bi, cap, B, scale_inv ? 1 : 0, pmn, pmx, scratch(aw, pts, (void*)ss).data_ptr(),
                                     (size_t)scratch(aw, pts, (void*)ss).numel(), (void*)ss),
                  "compute_aabb");
            ncs.assign(L, 1);
            if (scale_inv) {
                for (int l = 0; l < L; ++l)
                    check(mccnn_num_cells(nullptr, nullptr, B, (float)radii[l], 1, &ncs[l], nullptr), "num_cells");
            } else {
                // determineNumCells with an absolute cell size (sort_gpu.cu:410-419): ONE read-back of the extent for all levels
                check(mccnn_aabb_extent(pmn, pmx, &extent, (void*)ss), "aabb_extent");
                for (int l = 0; l < L; ++l) {
                    const int nc = (int)(extent / (float)radii[l]);
                    ncs[l] = nc ? nc : 1;
                }
            }
            size_t need = 256;
            std::vector<size_t> wsb(L);
            for (int l = 0; l < L; ++l) {
                wsb[l] = mccnn_hierarchy_level_workspace_bytes(cap, B, ncs[l]);
                if (!wsb[l]) throw std::runtime_error("PointHierarchy: batch_size * num_cells^3 does not fit 32-bit keys");
                wsb[l] = (wsb[l] + 255) / 256 * 256;
                const size_t tmp = (size_t)(5 * ca) * 4 + (size_t)2 * B * ncs[l] * ncs[l] * ncs[l] * 4;
                if (wsb[l] + tmp > need) need = wsb[l] + tmp;
            }
            Tensor& ws = scratch(need, pts, (void*)ss);
            int* sz = sizes.data_ptr<int>();
            hip_check(hipMemcpyAsync(sz, &cap, sizeof(int), hipMemcpyHostToDevice, ss), "hipMemcpyAsync");
            const float* cur_pts = P;
            const int* cur_bids = Bi;
            for (int l = 0; l < L; ++l) {
                char* base = (char*)ws.data_ptr();
                int* ti_ = (int*)(base + wsb[l]);           // index_new_pos | sorted batch ids | cell table
                float* tf_ = (float*)(ti_ + 2 * ca);        // sorted points
                int* cells = (int*)(tf_ + 3 * ca);
                int* bi = ints[l].data_ptr<int>();
                float* bf = flts[l].data_ptr<float>();
                check(mccnn_hierarchy_level(cur_pts, cur_bids, pmn, pmx, cap, sz + l, B, ncs[l], (float)radii[l],
                                            scale_inv ? 1 : 0, pmode, ti_, tf_, ti_ + ca, cells, bf, bi, bi + ca, bi + 2 * ca,
                                            sz + l + 1, base, wsb[l], (void*)ss),
                      "hierarchy_level");
                cur_pts = bf;
                cur_bids = bi;
            }
            static thread_local Tensor host;
            if (!host.defined() || host.numel() < L + 1)
                host = at::empty({L + 65}, at::TensorOptions().dtype(at::kInt).pinned_memory(true));
            hip_check(hipMemcpyAsync(host.data_ptr(), sz, (size_t)(L + 1) * sizeof(int), hipMemcpyDeviceToHost, ss), "hipMemcpyAsync");
            if (!feats.defined()) hip_check(hipEventRecord(event, ss), "hipEventRecord");
            hip_check(hipStreamSynchronize(ss), "hipStreamSynchronize");
            hs.assign(host.data_ptr<int>(), host.data_ptr<int>() + L + 1);
            for (int l = 1; l <= L; ++l)
                if (hs[l] < 0) {   // (rare and worth knowing: a wait of the single-launch Poisson kernel timed out under load)
                    fprintf(stderr, "mccnn: prefetched hierarchy: level %d gave up (size %d); the caller builds it op by op\n", l, hs[l]);
                    break;
                }
            if (feats.defined()) {
                bool ok = true;
                for (int l = 1; l <= L; ++l) ok = ok && hs[l] >= 0;
                const int words = (int)(feats.size(1) * (int64_t)feats.element_size() / 4);
                const float* src = (const float*)feats.data_ptr();
                for (int l = 0; ok && l < L; ++l) {   // rows of level l + 1 = rows of level l at transformedIndexs
                    check(mccnn_permute_gather(src, ints[l].data_ptr<int>() + 2 * ca, hs[l + 1], words,
                                               (float*)lfeats[l].data_ptr(), (void*)ss), "permute_gather");
                    src = (const float*)lfeats[l].data_ptr();
                }
                hip_check(hipEventRecord(event, ss), "hipEventRecord");
            }
            if (mccnn::debug_int("hier_trace", 0)) {
                std::string line = "hier job: cap " + std::to_string(cap) + " extent " + std::to_string(extent) + " nc";
                for (int l = 0; l < L; ++l) line += " " + std::to_string(ncs[l]);
                line += " sizes";
                for (int l = 0; l <= L; ++l) line += " " + std::to_string(hs[l]);
                fprintf(stderr, "%s\n", line.c_str());
            }
        } catch (const std::exception& e) {
            rc = 1;
            what = e.what();
        }
        done.store(1, std::memory_order_release);
    }

    // -> (aabbMin, aabbMax, extent, levels) on the calling thread's current stream; levels empty when a wait of the
    // single-launch Poisson kernel timed out (the caller then builds the hierarchy op by op)
    py::tuple result() {
        {
            py::gil_scoped_release nogil;
            const auto t0 = std::chrono::steady_clock::now();
            wait_done();
            g_wait_ns.fetch_add(std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count(),
                                std::memory_order_relaxed);
        }
        if (rc) throw std::runtime_error("PointHierarchy prefetch: " + what);
        const DevGuard device_guard((int)pts.device().index());
        if (!joined) {
            void* consumer_stream = cur_stream(pts);
            hip_check(hipStreamWaitEvent((hipStream_t)consumer_stream, event, 0), "hipStreamWaitEvent");
            joined = true;
            // (allocated on the hierarchy's stream, consumed on this one from here on)
            const c10::Stream consumer = as_torch_stream(consumer_stream, (int)pts.device().index());
            if (block.defined()) {
                block.record_stream(consumer);   // (every output is a view of it)
            } else {
                mn.record_stream(consumer);
                mx.record_stream(consumer);
                for (Tensor& t : ints) t.record_stream(consumer);
                for (Tensor& t : flts) t.record_stream(consumer);
                for (Tensor& t : lfeats) t.record_stream(consumer);
            }
        }
        std::vector<std::vector<Tensor>> out;
        bool ok = true;
        for (int l = 1; l <= L; ++l) ok = ok && hs[l] >= 0;
        for (int l = 0; ok && l < L; ++l) {
            const int64_t sN = hs[l + 1];
            out.push_back({flts[l].narrow(0, 0, 3 * sN).view({sN, 3}), ints[l].narrow(0, 0, sN).view({sN, 1}),
                           ints[l].narrow(0, ca, sN), ints[l].narrow(0, 2 * ca, sN)});
            if (feats.defined()) {   // 5th entry: the level's feature rows
                const int64_t F = feats.size(1);
                out.back().push_back(lfeats[l].narrow(0, 0, sN * F).view({sN, F}));
            }
        }
        return py::make_tuple(mn, mx, extent, out);
    }
};

hipEvent_t hierarchy_ready_event(const std::shared_ptr<HierFuture>& f) {
    return (f && f->joined && f->rc == 0 && f->done.load(std::memory_order_acquire)) ? f->event : nullptr;
}
bool hierarchy_owns(const std::shared_ptr<HierFuture>& f, const Tensor& t) {
    if (!f || !t.defined() || !t.is_cuda()) return false;
    const char* p = static_cast<const char*>(t.data_ptr());
    auto inside = [p](const Tensor& o) {
        if (!o.defined() || !o.is_cuda()) return false;
        const char* b = static_cast<const char*>(o.data_ptr());
        return p >= b && p < b + o.nbytes();
    };
    if (inside(f->pts) || inside(f->bids) || inside(f->mn) || inside(f->mx)) return true;
    for (const Tensor& o : f->ints) if (inside(o)) return true;
    for (const Tensor& o : f->flts) if (inside(o)) return true;
    for (const Tensor& o : f->lfeats) if (inside(o)) return true;
    return false;
}

// after_mode: 0 = the build starts behind everything the calling stream holds now (where the inputs were produced);
// 1 = the inputs are complete (uploaded and synchronised, or resident for long): the build starts at once;
// 2 = behind `after_event` (a hipEvent_t: the upload's own stream recorded it).
std::shared_ptr<HierFuture> hierarchy_prefetch(const Tensor& pts, const Tensor& bids, const std::vector<double>& radii,
                                               int64_t B, bool scale_inv, int64_t pmode, int64_t after_mode,
                                               int64_t after_event, const c10::optional<Tensor>& feats) {
    check_dev(pts, at::kFloat, "points");
    check_dev(bids, at::kInt, "batch ids");
    const DevGuard device_guard((int)pts.device().index());
    const int L = (int)radii.size();
    const int cap = (int)pts.size(0);
    TORCH_CHECK(L > 0 && cap > 0 && B > 0, "hierarchy_prefetch: bad arguments");
    hipStream_t ss = hier_stream();
    TORCH_CHECK(ss, "hierarchy_prefetch: no side stream");
    auto f = std::make_shared<HierFuture>();
    f->pts = pts; f->bids = bids; f->radii = radii;
    f->B = (int)B; f->L = L; f->cap = cap; f->pmode = (int)pmode; f->scale_inv = scale_inv;
    f->ca = (cap + 63) / 64 * 64;
    auto iopt = pts.options().dtype(at::kInt);
    void* stream = cur_stream(pts);
    {
        // the outputs come from the caching allocator's pool of the hierarchy's OWN stream: a block it hands out was last
        // used on that stream, so the build needs no ordering behind the calling stream for its memory (only for its
        // inputs, below); result() tells the allocator about the stream that consumes them (record_stream)
        const c10::hip::HIPStreamGuardMasqueradingAsCUDA own(as_torch_stream((void*)ss, (int)pts.device().index()));
        bool with_feats = false;
        if (feats.has_value() && feats->defined()) {
            const Tensor& ft = *feats;
            // short rows without a gradient only (the input features of a network: ones, normals, colours): the level
            // buffers are sized by the capacity
            const int64_t row_bytes = ft.dim() == 2 ? ft.size(1) * (int64_t)ft.element_size() : 0;
            with_feats = ft.is_cuda() && ft.device() == pts.device() && ft.dim() == 2 && ft.size(0) == cap && ft.is_contiguous() &&
                         !ft.requires_grad() && row_bytes > 0 && row_bytes <= 256 && row_bytes % 4 == 0 &&
                         (ft.scalar_type() == at::kFloat || ft.scalar_type() == at::kBFloat16);
            if (with_feats) f->feats = ft;
        }
        // ONE block for everything the hierarchy hands out (boxes, level sizes, every level's rows): a block that carries
        // record_stream() costs its consumer's QUEUE an event record when it is freed (~3-5 us of queue time each; a dozen
        // blocks per hierarchy were 0.08 ms of the calling queue per step of BASELINE cfg4) -- one block, one record
        auto al = [](int64_t b) { return (b + 255) / 256 * 256; };
        const int64_t bBox = al(B * 3 * 4), bSz = al((L + 1) * 4), bLvl = al(3 * f->ca * 4);
        const int64_t bFt = with_feats ? al(f->ca * f->feats.size(1) * (int64_t)f->feats.element_size()) : 0;
        f->block = at::empty({2 * bBox + bSz + L * (2 * bLvl + bFt)}, pts.options().dtype(at::kByte));
        int64_t off = 0;
        auto piece = [&](int64_t bytes, int64_t used, at::ScalarType dt) {
            Tensor t = f->block.narrow(0, off, used).view(dt);
            off += bytes;
            return t;
        };
        f->mn = piece(bBox, B * 3 * 4, at::kFloat).view({B, 3});
        f->mx = piece(bBox, B * 3 * 4, at::kFloat).view({B, 3});
        f->sizes = piece(bSz, (L + 1) * 4, at::kInt);
        for (int l = 0; l < L; ++l) {
            f->ints.push_back(piece(bLvl, 3 * f->ca * 4, at::kInt));
            f->flts.push_back(piece(bLvl, 3 * f->ca * 4, at::kFloat));
            if (with_feats)
                f->lfeats.push_back(piece(bFt, f->ca * f->feats.size(1) * (int64_t)f->feats.element_size(), f->feats.scalar_type()));
        }
    }
    f->alloc_stream = (void*)ss;
    f->event = take_event();
    if (after_mode == 2 && after_event) {
        hip_check(hipStreamWaitEvent(ss, (hipEvent_t)(uintptr_t)after_event, 0), "hipStreamWaitEvent");
    } else if (after_mode != 1) {
        static thread_local hipEvent_t fork_ev = nullptr;
        if (!fork_ev) hip_check(hipEventCreateWithFlags(&fork_ev, hipEventDisableTiming), "hipEventCreate");
        hip_check(hipEventRecord(fork_ev, (hipStream_t)stream), "hipEventRecord");
        hip_check(hipStreamWaitEvent(ss, fork_ev, 0), "hipStreamWaitEvent");
    }
    if (Issuer::enabled()) {
        f->done.store(0, std::memory_order_release);
        Issuer::get(1).push([f, ss] { f->run(ss); });
    } else {
        f->run(ss);
    }
    return f;
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, mod) {
    mod.doc() = "PyTorch-ROCm side of the native step executor of libmccnn_hip.so";
    if (mccnn::debug_int("trace_terminate", 0)) {   // debugging: where std::terminate was called from
        std::set_terminate([] {
            void* frames[64];
            const int n = backtrace(frames, 64);
            backtrace_symbols_fd(frames, n, 2);
            abort();
        });
    }
    static py::exception<CapacityError> cap_exc(mod, "CapacityError");
    py::register_exception_translator([](std::exception_ptr p) {
        try {
            if (p) std::rethrow_exception(p);
        } catch (const CapacityError& e) {
            PyErr_SetObject(cap_exc.ptr(), py::int_(e.edges).ptr());
        }
    });
    py::class_<Geo, std::shared_ptr<Geo>>(mod, "Geometry")
        .def_readonly("buf", &Geo::buf)
        .def_readonly("n", &Geo::n)
        .def_readonly("m", &Geo::m)
        .def_readonly("nc", &Geo::nc)
        .def_readonly("B", &Geo::B)
        .def_readonly("e_cap", &Geo::e_cap)
        .def_property_readonly("e", [](const Geo& g) { return g.e.load(std::memory_order_relaxed); })
        .def_readonly("grid_owner", &Geo::grid_owner)
        .def_readwrite("uses", &Geo::uses)
        .def_readonly("side", &Geo::side)
        .def_readonly("have", &Geo::have)
        .def_readonly("point", &Geo::pp)
        // (none of the calls below touches a Python object, and all of them may wait -- for a helper thread's job, which can
        // in turn wait for a device-side edge total, or for the device itself: the GIL is released for their whole
        // duration, so data-loader threads keep running and a helper thread that drops the last reference to a tensor
        // with a Python wrapper can take the GIL in its destructor instead of dead-locking against a spinning caller)
        .def("join", [](Geo& g, const at::Tensor& like) { g.join(cur_stream(like)); }, py::call_guard<py::gil_scoped_release>())
        .def("prebuild", &Geo::prebuild, py::arg("what"), py::arg("avg"), py::arg("side"), py::arg("like"),
             py::call_guard<py::gil_scoped_release>())
        .def("edges", &Geo::edges, py::arg("wait_us") = -1, py::call_guard<py::gil_scoped_release>())
        .def("info", &Geo::info, py::call_guard<py::gil_scoped_release>())
        .def("cap_addr", &Geo::cap_addr, py::call_guard<py::gil_scoped_release>())
        // (avg of the per-edge records the geometry holds or -1, their device address or 0)
        .def("records", [](Geo& g) {
            g.wait_issued();
            const void* p = nullptr;
            const int avg = mccnn_geometry_records(g.h, &p);
            return std::make_pair(avg, (int64_t)(uintptr_t)p);
        }, py::call_guard<py::gil_scoped_release>());
    py::class_<PointPdf, std::shared_ptr<PointPdf>>(mod, "PointPdf")
        .def_readonly("density", &PointPdf::density)
        .def_readonly("counts", &PointPdf::counts)
        // whoever reads the tensors does so on the current stream: behind the sweep, known to the density's allocator
        .def("join", [](PointPdf& p) { p.order(cur_stream(p.density)); }, py::call_guard<py::gil_scoped_release>());
    mod.def("build_geometry", &build_geometry, py::arg("pts"), py::arg("bids"), py::arg("centres"), py::arg("cbids"),
            py::arg("mn"), py::arg("mx"), py::arg("B"), py::arg("nc"), py::arg("radius"), py::arg("scale_inv"),
            py::arg("window"), py::arg("use_pdf"), py::arg("capacity"), py::arg("grid_from").none(true),
            py::arg("side") = -1, py::arg("fork") = false, py::arg("background") = false,
            py::arg("after").none(true) = py::none(), py::arg("max_neighbors") = 0, py::arg("sample_seed") = -1,
            py::arg("point_pdf") = false, py::arg("point_from").none(true) = py::none(), py::arg("max_edges") = 0,
            py::arg("records_avg") = -1, py::call_guard<py::gil_scoped_release>());
    mod.def("sampled_features", &sampled_features, py::call_guard<py::gil_scoped_release>());
    mod.def("begin_geometry_batch", &begin_geometry_batch);
    mod.def("end_geometry_batch", &end_geometry_batch, py::call_guard<py::gil_scoped_release>());
    mod.def("prebuild_async", &prebuild_async, py::arg("geometry"), py::arg("what"), py::arg("avg"),
            py::call_guard<py::gil_scoped_release>());
    mod.def("conv", &conv, py::arg("geometry"), py::arg("feats"), py::arg("w1"), py::arg("b1"), py::arg("w2"), py::arg("b2"),
            py::arg("w3"), py::arg("b3"), py::arg("fout"), py::arg("combin"), py::arg("avg"), py::arg("deterministic") = false,
            py::call_guard<py::gil_scoped_release>());
    mod.def("bn_relu_drop", &bn_relu_drop, py::arg("x"), py::arg("gamma"), py::arg("beta"), py::arg("moving_mean"),
            py::arg("moving_var"), py::arg("training"), py::arg("relu"), py::arg("keep_threshold"), py::arg("keep_scale"),
            py::arg("seed"), py::arg("momentum"), py::arg("epsilon"), py::arg("out_type") = -1, py::call_guard<py::gil_scoped_release>());
    mod.def("bn_relu_drop_cat", &bn_relu_drop_cat, py::arg("xs"), py::arg("gamma"), py::arg("beta"), py::arg("moving_mean"),
            py::arg("moving_var"), py::arg("training"), py::arg("relu"), py::arg("keep_threshold"), py::arg("keep_scale"),
            py::arg("seed"), py::arg("momentum"), py::arg("epsilon"), py::arg("out_type") = -1, py::call_guard<py::gil_scoped_release>());
    mod.def("bn_sync_stats", &bn_sync_stats, py::call_guard<py::gil_scoped_release>());
    mod.def("bn_sync_apply", &bn_sync_apply, py::call_guard<py::gil_scoped_release>());
    mod.def("bn_sync_bwd_sums", &bn_sync_bwd_sums, py::call_guard<py::gil_scoped_release>());
    mod.def("bn_sync_bwd_dx", &bn_sync_bwd_dx, py::call_guard<py::gil_scoped_release>());
    mod.def("linear_bn_relu_drop", &linear_bn_relu_drop, py::arg("x"), py::arg("w"), py::arg("b"), py::arg("gamma"), py::arg("beta"),
            py::arg("moving_mean"), py::arg("moving_var"), py::arg("training"), py::arg("relu"), py::arg("keep_threshold"),
            py::arg("keep_scale"), py::arg("seed"), py::arg("momentum"), py::arg("epsilon"), py::arg("out_type") = -1,
            py::call_guard<py::gil_scoped_release>());
    mod.def("linear_softmax_xent", &linear_softmax_xent, py::arg("x"), py::arg("w"), py::arg("b"), py::arg("labels"),
            py::arg("weights") = py::none(), py::arg("want_logits") = false, py::call_guard<py::gil_scoped_release>());
    mod.def("cosine_distance_loss", &cosine_distance_loss, py::arg("pred"), py::arg("target"), py::arg("weights") = py::none(),
            py::call_guard<py::gil_scoped_release>());
    mod.def("segmentation_counts", &segmentation_counts, py::arg("pred"), py::arg("labels"), py::arg("num_classes"),
            py::arg("batch_ids") = py::none(), py::arg("num_clouds") = 1, py::arg("weights") = py::none(),
            py::arg("ignore_label") = -1, py::arg("out") = py::none(), py::call_guard<py::gil_scoped_release>());
    mod.def("voxel_counts", &voxel_counts, py::arg("points"), py::arg("pred"), py::arg("labels"), py::arg("num_classes"),
            py::arg("batch_ids"), py::arg("num_clouds"), py::arg("aabb_min"), py::arg("resolution"), py::arg("ignore_label"),
            py::arg("max_ignore_share"), py::arg("out") = py::none(), py::arg("dropped") = py::none(), py::arg("ws") = py::none(),
            py::call_guard<py::gil_scoped_release>());
    mod.def("compute_aabb", &compute_aabb);
    mod.def("hierarchy_levels", &hierarchy_levels, py::call_guard<py::gil_scoped_release>());
    py::class_<HierFuture, std::shared_ptr<HierFuture>>(mod, "HierarchyFuture")
        .def("result", &HierFuture::result)
        .def("done", [](HierFuture& f) { return f.done.load(std::memory_order_acquire) != 0; });
    mod.def("hierarchy_prefetch", &hierarchy_prefetch, py::arg("pts"), py::arg("bids"), py::arg("radii"), py::arg("B"),
            py::arg("scale_inv"), py::arg("pmode"), py::arg("after_mode") = 0, py::arg("after_event") = 0,
            py::arg("feats") = py::none(), py::call_guard<py::gil_scoped_release>());
    mod.def("shutdown_helpers", [] { for (int k = 0; k < 3; ++k) Issuer::get(k).retire(); },
            py::call_guard<py::gil_scoped_release>());
    mod.def("wait_ns", [] { return (long long)g_wait_ns.load(std::memory_order_relaxed); });
    mod.def("debug_counters", [] {
        py::dict d;
        d["caller_orderings"] = (long long)g_caller_orderings.load(std::memory_order_relaxed);
        return d;
    });
    mod.def("debug_times", [](bool reset) {
        static const char* names[T_N] = {"fwd", "fwd_lib", "fwd_alloc", "bwd", "bwd_lib", "bwd_alloc", "bwd_views", "bwd_join"};
        py::dict d;
        for (int k = 0; k < T_N; ++k) {
            d[names[k]] = py::make_tuple((long long)g_t_ns[k].load(), (long long)g_t_calls[k].load());
            if (reset) { g_t_ns[k].store(0); g_t_calls[k].store(0); }
        }
        return d;
    }, py::arg("reset") = false);
}
