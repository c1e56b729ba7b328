// rl_api.hip -- implementation of include/robigo_luculenta.h over the gfx950 kernels.
//
// Ordering model: every trace, plot and gather unit owns a NON-blocking HIP stream and nothing relies on the
// null stream's implicit ordering (RCCL and a host framework's side streams are non-blocking too).  Every
// hand-over between units is an event, recorded on the stream that gives and waited for on the stream that takes
// (`hand_over` below; each call site says why it is there):
//   * a fused render writes the plot unit's buffer from the trace unit's stream: the plot stream waits for it
//     (so "everything written into this plot unit so far" is always the tail of the plot unit's own stream),
//     and the render itself waits for the plot unit's last clear;
//   * PlotUnit::plot reads mapped_photons on the plot stream after the trace unit's render; the trace unit's
//     next render waits for that plot;
//   * GatherUnit::accumulate runs on the gather stream after the plot stream's tail, and the plot stream
//     continues after the clear; tonemap kernels run on the gather stream;
//   * the GatherUnit-time exchange (rl_plot_unit_reduce, RCCL) is enqueued on the plot stream.
//   * the blocking render calls (open launches, see `Session` below) are ordered on the HOST instead: before a call
//     is appended to a kernel that is already running, the host waits for whatever still reads or clears its target,
//     and the call (or whoever ends a begun one) returns only when the kernel has reported its last path.
// Downloads synchronise the stream that produced the data (`download`, `upload`).  Trace and plot work of different
// units overlap on the device.  The streams, events and device memory of a handle are held by its `Ledger`, whose
// release drains the handle's streams before anything they may still use is destroyed or freed: a *_destroy ends what
// only the unit knows of (a begun render), then releases.  Entry points never throw.
#include <hip/hip_runtime.h>
#include <sys/prctl.h>

#include <dlfcn.h>
#include <unistd.h> // fsync

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include <rccl/rccl.h> // types and prototypes only: the library is bound at run time (rccl_api below)

#include "../../include/robigo_luculenta.h"
#include "../../include/robigo_luculenta_debug.h"
#include "rl_kernels.hip.h"
#include "rl_query.hip.h"
#include "rl_occlusion.hip.h"
#include "rl_film.hip.h"
#include "rl_paths.hip.h"
#include "rl_step.hip.h"
#include "rl_path_list.hip.h"
#include "rl_light.hip.h"
#include "rl_light_film.hip.h"
#include "rl_direct.hip.h"
#include "rl_features.hip.h"
#include "rl_denoise.hip.h"
#include "rl_spectral.hip.h"
#include "rl_relight.hip.h"
#include "rl_glare.hip.h"
#include "rl_error.hip.h"
#include "rl_robust.hip.h"
#include "rl_adaptive.hip.h"
#include "rl_scene.h"

namespace {

thread_local std::string g_error;

int fail(int code, const std::string& msg) {
    g_error = msg;
    return code;
}

} // namespace

// Internal (not in the C header): lets rl_app.cpp hand a worker thread's error message to the thread that
// called rl_app_run -- rl_last_error() is per thread.
void rl_internal_set_last_error(const std::string& msg) { g_error = msg; }

namespace {

#define RL_HIP(call)                                                                                        \
    do {                                                                                                    \
        hipError_t e_ = (call);                                                                             \
        if (e_ != hipSuccess)                                                                               \
            return fail(RL_E_HIP, std::string(#call) + ": " + hipGetErrorString(e_));                       \
    } while (0)

// RL_MAX_PIXELS (robigo_luculenta.h): checked before use_device, like the zero-size check.
int check_image_size(const char* unit, uint32_t width, uint32_t height) {
    if ((uint64_t)width * height <= RL_MAX_PIXELS) return RL_OK;
    return fail(RL_E_INVALID, std::string(unit) + ": " + std::to_string(width) + " x " + std::to_string(height) +
                                  " pixels exceed RL_MAX_PIXELS = 2^31 - 1 (the kernels index pixels in 32 bits)");
}

int use_device(int device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(RL_E_NO_DEVICE, "no HIP device is visible");
    if (device < 0 || device >= n) return fail(RL_E_INVALID, "device index out of range");
    RL_HIP(hipSetDevice(device));
    return RL_OK;
}

// A unit's own stream: non-blocking, so that it never waits for the null stream (RL_BLOCKING_STREAMS in the environment:
// measurement runs ask for a blocking one).
hipError_t create_unit_stream(hipStream_t* stream) {
    return hipStreamCreateWithFlags(stream, getenv("RL_BLOCKING_STREAMS") ? hipStreamDefault : hipStreamNonBlocking);
}

int cu_count_of(int device, int* out);
// What a call on a unit starts with once its arguments are checked: the unit's device current, and its CU count.
int enter_device(int device, int* cus) {
    const int rc = use_device(device);
    return rc != RL_OK ? rc : cu_count_of(device, cus);
}

// A unit handed to a call on another unit must live on the same device and have the same image size.
const char* unit_name(const RlTraceUnit*) { return "trace unit"; }
const char* unit_name(const RlPlotUnit*) { return "plot unit"; }
const char* unit_name(const RlGatherUnit*) { return "gather unit"; }
const char* unit_name(const RlTonemapUnit*) { return "tonemap unit"; }
const char* unit_name(const RlDenoiseUnit*) { return "denoise unit"; }
const char* unit_name(const RlSpectralUnit*) { return "spectral unit"; }
const char* unit_name(const RlRelightUnit*) { return "relight unit"; }
const char* unit_name(const RlGlareUnit*) { return "glare unit"; }
const char* unit_name(const RlErrorUnit*) { return "error unit"; }
const char* unit_name(const RlRobustUnit*) { return "robust unit"; }
const char* unit_name(const RlAdaptiveUnit*) { return "adaptive unit"; }
template <class Given, class Owner>
int match_check(const Given* given, const Owner* owner) {
    if (given->device == owner->device && given->width == owner->width && given->height == owner->height) return RL_OK;
    return fail(RL_E_STATE, std::string(unit_name(given)) + " does not match the " + unit_name(owner) + " (device or size)");
}

// The hand-over of the ordering model (top of the file): what is queued on `to` from here on runs behind everything queued on
// `from` so far.  `event` is recorded on `from` and waited for on `to`.
int hand_over(hipEvent_t event, hipStream_t from, hipStream_t to) {
    RL_HIP(hipEventRecord(event, from));
    RL_HIP(hipStreamWaitEvent(to, event, 0));
    return RL_OK;
}

// Returns when `stream` has drained, also after a failure: rc if it failed, else what the drain returned.  A call that queued
// work which reads or writes host memory, or buffers that may be freed next, leaves through this.
int drained(hipStream_t stream, int rc) {
    const hipError_t e = hipStreamSynchronize(stream);
    if (rc != RL_OK) return rc;
    RL_HIP(e);
    return RL_OK;
}

// Host copies of a unit's buffers, plane by plane (a null host pointer: that plane is skipped).  `stream` is the one that
// produced the data or still reads it, and drains first (null: nothing was ever queued).
struct Plane {
    void* dev;
    const void* host;
    size_t bytes;
};
int download(hipStream_t stream, std::initializer_list<Plane> planes) {
    if (stream) RL_HIP(hipStreamSynchronize(stream));
    for (const Plane& p : planes)
        if (p.host) RL_HIP(hipMemcpy(const_cast<void*>(p.host), p.dev, p.bytes, hipMemcpyDeviceToHost));
    return RL_OK;
}
int upload(hipStream_t stream, std::initializer_list<Plane> planes) {
    if (stream) RL_HIP(hipStreamSynchronize(stream));
    for (const Plane& p : planes)
        if (p.host) RL_HIP(hipMemcpy(p.dev, p.host, p.bytes, hipMemcpyHostToDevice));
    RL_HIP(hipStreamSynchronize(nullptr)); // (the null stream only: a resident open trace kernel of another unit is not waited for)
    return RL_OK;
}

struct EventPair {
    hipEvent_t start, stop;
};

// One launch on `stream` between the events of `pair`; *launches counts the launches that were accepted.  Whether and when the
// pair may be read is the caller's: the units differ in it (include/robigo_luculenta_debug.h).
void count_launch(std::atomic<uint64_t>* launches) { launches->fetch_add(1, std::memory_order_relaxed); }
void count_launch(uint64_t* launches) { *launches += 1; }
template <class Counter, class Launch>
int timed_launch(const EventPair& pair, hipStream_t stream, Counter* launches, Launch launch) {
    RL_HIP(hipEventRecord(pair.start, stream));
    launch();
    RL_HIP(hipGetLastError());
    RL_HIP(hipEventRecord(pair.stop, stream));
    count_launch(launches);
    return RL_OK;
}

// rl_debug_live_resources: what the ledgers of all live handles hold.  Fed by Ledger's acquire and release and by nothing else.
enum { LIVE_ALLOCATIONS, LIVE_STREAMS, LIVE_EVENTS, LIVE_PAIRS, LIVE_KINDS };
std::atomic<uint64_t> g_live[LIVE_KINDS];

// The device resources of one handle.  Every acquisition writes the raw pointer or handle into the field the caller names and
// records it here; after the first failure the later ones do nothing, so a *_create is a flat list and one check of finish().
// release() is the only code that destroys or frees what a handle holds, for a complete handle and a half-built one alike.
struct Ledger {
    std::vector<void*> memory;
    std::vector<hipStream_t> streams;
    std::vector<hipEvent_t> events;
    std::vector<EventPair> pairs;
    hipError_t error = hipSuccess; // the first failed acquisition
    bool filled = false;           // a synchronous memset or copy ran on the null stream

    // Device memory as it comes (fill = nullptr), or holding the `bytes` bytes at `fill`.
    template <class T>
    void alloc(T** field, size_t bytes, const void* fill = nullptr) {
        *field = nullptr;
        if (error != hipSuccess || (error = hipMalloc((void**)field, bytes)) != hipSuccess) return;
        memory.push_back((void*)*field);
        g_live[LIVE_ALLOCATIONS].fetch_add(1, std::memory_order_relaxed);
        if (fill) error = hipMemcpy((void*)*field, fill, bytes, hipMemcpyHostToDevice), filled = true;
    }
    template <class T>
    void alloc_zeroed(T** field, size_t bytes) {
        alloc(field, bytes);
        if (error == hipSuccess) error = hipMemset((void*)*field, 0, bytes), filled = true;
    }
    void stream(hipStream_t* field) {
        *field = nullptr;
        if (error != hipSuccess || (error = create_unit_stream(field)) != hipSuccess) return;
        streams.push_back(*field);
        g_live[LIVE_STREAMS].fetch_add(1, std::memory_order_relaxed);
    }
    // A plain event: it orders streams and is never timed.
    void event(hipEvent_t* field) {
        *field = nullptr;
        if (error != hipSuccess || (error = hipEventCreateWithFlags(field, hipEventDisableTiming)) != hipSuccess) return;
        events.push_back(*field);
        g_live[LIVE_EVENTS].fetch_add(1, std::memory_order_relaxed);
    }
    // Device memory and a plain event for a live handle, taken at the first call that needs them: as make_pair, the failure is
    // the call's, not the handle's.
    template <class T>
    hipError_t make_alloc(T** field, size_t bytes) {
        *field = nullptr;
        const hipError_t e = hipMalloc((void**)field, bytes);
        if (e != hipSuccess) return e;
        memory.push_back((void*)*field);
        g_live[LIVE_ALLOCATIONS].fetch_add(1, std::memory_order_relaxed);
        return hipSuccess;
    }
    hipError_t make_event(hipEvent_t* field) {
        *field = nullptr;
        const hipError_t e = hipEventCreateWithFlags(field, hipEventDisableTiming);
        if (e != hipSuccess) return e;
        events.push_back(*field);
        g_live[LIVE_EVENTS].fetch_add(1, std::memory_order_relaxed);
        return hipSuccess;
    }
    // A timed pair.  make_pair is the form for a live handle (PairPool): its failure is the call's, not the handle's.
    hipError_t make_pair(EventPair* field) {
        *field = EventPair{nullptr, nullptr};
        hipError_t e = hipEventCreate(&field->start);
        if (e == hipSuccess && (e = hipEventCreate(&field->stop)) != hipSuccess) (void)hipEventDestroy(field->start);
        if (e != hipSuccess) return e;
        pairs.push_back(*field);
        g_live[LIVE_PAIRS].fetch_add(1, std::memory_order_relaxed);
        return hipSuccess;
    }
    void pair(EventPair* field) {
        if (error == hipSuccess) error = make_pair(field);
    }
    // The end of a *_create: the first failure, if any.
    hipError_t finish() {
        if (error == hipSuccess && filled) error = hipStreamSynchronize(nullptr); // the synchronous memsets and copies ran on the null stream (that stream only: a resident open trace kernel of another unit is not waited for)
        return error;
    }
    // Device current.  The streams drain before anything they may still use goes.
    void release() {
        for (hipStream_t s : streams) (void)hipStreamSynchronize(s);
        for (hipStream_t s : streams) (void)hipStreamDestroy(s);
        for (hipEvent_t e : events) (void)hipEventDestroy(e);
        for (const EventPair& p : pairs) (void)hipEventDestroy(p.start), (void)hipEventDestroy(p.stop);
        for (void* p : memory) (void)hipFree(p);
        g_live[LIVE_ALLOCATIONS].fetch_sub(memory.size(), std::memory_order_relaxed);
        g_live[LIVE_STREAMS].fetch_sub(streams.size(), std::memory_order_relaxed);
        g_live[LIVE_EVENTS].fetch_sub(events.size(), std::memory_order_relaxed);
        g_live[LIVE_PAIRS].fetch_sub(pairs.size(), std::memory_order_relaxed);
        memory.clear(), streams.clear(), events.clear(), pairs.clear();
    }
};

// Timed pairs around work on a stream whose milliseconds are read later, if ever.  The pairs are the ledger's; the pool only
// says where each one is: spare, taken by a call, or pending (recorded around work, not read yet; oldest first).
struct PairPool {
    std::vector<EventPair> pending, spare;
    int take(Ledger* ledger, EventPair* pair) {
        if (spare.empty()) {
            RL_HIP(ledger->make_pair(pair));
        } else {
            *pair = spare.back();
            spare.pop_back();
        }
        return RL_OK;
    }
    void give_back(const EventPair& pair) { spare.push_back(pair); }
    // Waits for the `n` oldest pending pairs, adds their milliseconds to *ms and their number to *count, and spares them.
    int harvest(size_t n, double* ms, uint64_t* count) {
        size_t done = 0;
        hipError_t e = hipSuccess;
        for (n = std::min(n, pending.size()); done < n; ++done) {
            float t = 0.0f;
            if ((e = hipEventSynchronize(pending[done].stop)) != hipSuccess) break;
            if ((e = hipEventElapsedTime(&t, pending[done].start, pending[done].stop)) != hipSuccess) break;
            *ms += (double)t;
            *count += 1;
            spare.push_back(pending[done]);
        }
        pending.erase(pending.begin(), pending.begin() + (long)done);
        if (e != hipSuccess) return fail(RL_E_HIP, std::string("event pair harvest: ") + hipGetErrorString(e));
        return RL_OK;
    }
};

// What the *_unit_create calls share.  unit_new: the argument checks in the header's order -- null output, zero size (`count`:
// whatever else must not be 0), RL_MAX_PIXELS, then the device -- and the handle with its device and size set.  unit_created:
// the one check behind the flat list of acquisitions; `destroy` is the unit's own, for a half-built handle as for a whole one.
template <class Unit>
int unit_new(const char* name, int device, uint32_t width, uint32_t height, uint32_t count, Unit** out, Unit** unit) {
    if (!out) return fail(RL_E_INVALID, "null output handle");
    *out = nullptr;
    if (width == 0 || height == 0 || count == 0) return fail(RL_E_INVALID, std::string("zero-sized ") + name);
    int rc = check_image_size(name, width, height);
    if (rc == RL_OK) rc = use_device(device);
    if (rc != RL_OK) return rc;
    Unit* u = new (std::nothrow) Unit();
    if (!u) return fail(RL_E_INVALID, "out of host memory");
    u->device = device;
    u->width = width;
    u->height = height;
    *unit = u;
    return RL_OK;
}
template <class Unit>
int unit_created(const char* what, Unit* u, int (*destroy)(Unit*), Unit** out) {
    const hipError_t e = u->ledger.finish();
    if (e != hipSuccess) {
        destroy(u);
        return fail(RL_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
    }
    *out = u;
    return RL_OK;
}

} // namespace

struct RlScene {
    int device;
    Ledger ledger; // blob, emitters, emitter_flags
    RlF4* blob;
    RlSceneLayout lay;
    size_t staged_bytes; // the whole blob
    size_t tables_bytes; // its tables: records [off_planes, off_objects)
    // The sampleable emitters (rl_scene_emitters, rl_scene_light_paths*): a device buffer of its own beside the blob,
    // RL_EMITTER_STRIDE records each, and their object indices in scan order.  Null and empty for a scene without one.
    RlF4* emitters;
    std::vector<uint32_t> emitter_objects;
    // One byte per object beside the table, 1 for the objects above (rl_plot_unit_light_paths*: whether a path ended on a light
    // that is sampled is decided per lane without a search).  Null for a scene without one.
    uint8_t* emitter_flags;
};

namespace {
struct Session;
enum { RL_SESSIONS_PINNED = 1000 }; // internal: session_begin found every open-launch slot held by begun renders

// Paths and segments of a trace unit's calls that open launches served.  Shared with the tickets of the fused renders
// begun on the unit, which are ended on other threads (whoever uses the plot unit next) and possibly after the unit is gone.
struct UnitCounters {
    std::atomic<uint64_t> paths{0}, segments{0};
    std::atomic<uint64_t> kernel_ns{0}; // the unit's share (by paths) of the open launches that carried its calls
};

// A blocking render that was begun and not yet ended.  The ticket of an un-fused render lives in its trace unit (whose
// photons it fills), that of a fused render in the PLOT unit it splats into: the trace unit only lends its image size
// and fetch mode and is free for the next call -- on whatever thread -- at once, so the ticket holds nothing of it but
// the counters to credit.
struct Ticket {
    bool pending = false;
    Session* session = nullptr; // the open launch the call was appended to; null: a plain launch (ragged or huge batch)
    uint32_t job = 0;
    uint64_t paths = 0;
    int device = 0;
    std::shared_ptr<UnitCounters> counters;
    double presync_us = 0.0, admit_us = 0.0;
};
}

// rl_wavelength_table_create: the table of rl_wavelength.h on a device, and the host's copy of it.
struct RlWavelengthTable {
    int device;
    uint64_t id;   // never 0, never reused: the open launches' key (an address may be, by the next table)
    Ledger ledger; // table
    float* table;  // RL_WAVELENGTH_TABLE_FLOATS floats: the quantiles, then the weights
    float host[RL_WAVELENGTH_TABLE_FLOATS];
};

struct RlTraceUnit {
    int device;
    uint32_t id, width, height, n_photons;
    const RlWavelengthTable* wavelengths; // rl_trace_unit_set_wavelengths: the caller's, null = the reference's uniform draw
    RlMappedPhoton* photons;
    unsigned long long* queue; // 3 counters, see rl_trace_kernel
    hipStream_t stream;
    hipEvent_t rendered; // recorded on `stream` after everything that fills this unit's photons
    int fetch;
    int cu_count;
    Ledger ledger;  // photons, queue, stream, rendered, and the pairs of `timed`
    PairPool timed; // around every launch_trace on `stream`; harvested into kernel_ms
    double kernel_ms;
    uint64_t launches;
    size_t tuned_dyn;  // launch configuration last set up for this unit: dynamic LDS bytes,
    const void* tuned_kernel; // kernel instantiation,
    int tuned_per_cu;  // resident workgroups per CU (0 = not set up yet)
    std::shared_ptr<UnitCounters> counters = std::make_shared<UnitCounters>(); // of this unit's calls that open launches served
    Ticket ticket;                                                               // rl_trace_unit_render_begin
};

struct RlPlotUnit {
    int device;
    uint32_t id, width, height;
    float* xyz; // the unit's own, or the caller's (rl_plot_unit_create: external_xyz, which the ledger does not hold)
    RlF4* cie;
    hipStream_t stream; // rl_plot_kernel launches, clears, the RCCL exchange; its tail = every write into xyz so far
    hipEvent_t plotted; // recorded after the last plot kernel of a PlotUnit::plot call
    hipEvent_t ready;   // recorded on `stream` when a gather (or a reader on another stream) takes the buffer
    hipEvent_t cleared; // recorded on the gather stream after accumulate + clear
    hipEvent_t tail;    // scratch: recorded on `stream` by a fused launch that has to start behind everything queued there
    Ledger ledger;
    PairPool exchanges; // around every rl_plot_unit_reduce on `stream`; pending until read (rl_plot_unit_exchange_stats)
    uint64_t exchange_count = 0;
    double exchange_ms = 0.0;
    Ticket ticket;      // rl_trace_unit_render_fused_begin: ended by whatever uses the buffer next (plot_settle)
};

struct RlGatherUnit {
    int device;
    uint32_t width, height;
    float* acc;
    float* comp;
    hipStream_t stream; // accumulate and tonemap kernels
    Ledger ledger;
    PairPool timed;     // rl_debug_gather_accumulate_ms
};

struct RlTonemapUnit {
    int device;
    uint32_t width, height;
    uint8_t* rgb;
    float* srgb;
    float* max_intensity;
    hipStream_t last_stream; // the gather stream the last tonemap ran on (downloads wait for it)
    Ledger ledger;
};

struct RlDenoiseUnit {
    int device;
    uint32_t width, height;
    RlF4* guides;        // RL_DENOISE_GUIDE_WORDS words per pixel (rl_denoise_guides_kernel)
    float* pingpong[2];  // C_1, C_2, ... of a call with more than one pass: width x height x 3 floats each
    hipEvent_t ready[4]; // recorded on the streams of the gather units a call reads: image, albedo, normal, aux
    EventPair timed[1 + RL_DENOISE_MAX_ITERATIONS]; // around the guide launch and each pass of the last call (rl_debug_denoise_pass_ms)
    uint32_t timed_passes; // passes of the last call that completed
    // rl_denoise_unit_denoise_variance, taken at the first such call (null before it):
    float* variance[2];       // V_0, V_1, ... ping-pong: width x height floats each
    hipEvent_t error_ready;   // recorded on the error unit's stream
    EventPair timed_variance; // around the V_0 launch of the last variance call (rl_debug_denoise_variance_ms)
    bool timed_variance_done; // ... of a call that completed
    Ledger ledger;
};

struct RlSpectralUnit {
    int device;
    uint32_t width, height, n_nodes;
    float spacing;      // 400.0f / (float)(n_nodes - 1): the nodes sit at 380.0f + (float)b * spacing
    float* film;        // n_nodes planes of width x height floats, node-major
    float* matrix;      // the n_nodes x 3 matrix of the projection in flight (RL_SPECTRAL_MAX_NODES x 3 floats)
    hipStream_t stream; // clears and splats; every splat call returns with it drained
    hipEvent_t ready;   // recorded on `stream` when a projection takes the film
    EventPair timed[2]; // around the last splat launch and the last projection launch (rl_debug_spectral_ms)
    bool timed_done[2]; // ... of a call that completed
    Ledger ledger;
};

struct RlRelightUnit {
    int device;
    uint32_t width, height, n_nodes, n_groups;
    uint32_t n_objects;     // of the table on the device; 0: no table yet (rl_relight_unit_set_groups)
    float spacing;          // 400.0f / (float)(n_nodes - 1), the spectral film's
    float* film;            // n_groups * n_nodes planes of width x height floats: plane g * n_nodes + b
    float* matrix;          // the composed (n_groups * n_nodes) x 3 matrix of the mix in flight
    uint8_t* groups;        // the table: one byte per object, room for groups_room of them
    uint32_t groups_room;
    // rl_relight_unit_render's scratch, taken at the first such call (null before it): RL_QUERY_CHUNK records each
    RlCameraSample* samples;
    RlSpectralRay* rays;
    RlPathResult* results;
    hipStream_t stream;     // clears, splats and renders; every splat and render call returns with it drained
    hipEvent_t ready;       // recorded on `stream` when a mix takes the film
    EventPair timed[3];     // around the last splat launch, the last path launch of a render and the last mix launch (rl_debug_relight_ms)
    bool timed_done[3];     // ... of a call that completed
    Ledger ledger;
};

struct RlGlareUnit {
    int device;
    uint32_t width, height, n_nodes, taps;
    uint32_t has_tables; // rl_glare_unit_set_kernels has put tables on the device
    bool exact_skip;     // ... with a NaN or an infinity among them: the kernel form that skips a tap outside the film
    float* tables;       // n_nodes tables of taps x taps floats, node-major
    float* matrix;       // the n_nodes x 3 matrix of the apply in flight
    hipStream_t stream;  // the table copies
    hipEvent_t ready;    // recorded on `stream` when an apply takes the tables
    EventPair timed;     // around the last apply's launch (rl_debug_glare_ms)
    bool timed_done;     // ... of a call that completed
    Ledger ledger;
};

// tests/test_glare.py writes a stand-in handle's first fields at these offsets (the checks that read a handle before any device
// work): a field that moves must move there too.
static_assert(offsetof(RlGlareUnit, width) == 4 && offsetof(RlGlareUnit, height) == 8 && offsetof(RlGlareUnit, n_nodes) == 12 &&
                  offsetof(RlGlareUnit, taps) == 16 && offsetof(RlGlareUnit, has_tables) == 20 && offsetof(RlSpectralUnit, n_nodes) == 12,
              "tests/test_glare.py: test_apply_checks_a_stand_in_handle_in_the_stated_order");

struct RlErrorUnit {
    int device;
    uint32_t width, height, tiles_x, tiles_y;
    double* sum_y;         // S: width x height doubles in rows
    double* sum_q;         // Q: the same
    float* se;             // the estimate's per-pixel result, width x height floats
    double* tiles;         // the estimate's {t_se, t_y} per tile, tiles in raster order
    uint64_t observations; // k
    uint64_t paths;        // N
    hipStream_t stream;    // clears, observes and estimates
    hipEvent_t observed;   // recorded on `stream` after an observe kernel: the plot unit's stream waits for it
    EventPair timed[2];    // around the last observe launch and the last estimate launch (rl_debug_error_ms)
    bool timed_done[2];    // ... recorded at least once
    Ledger ledger;
};

struct RlRobustUnit {
    int device;
    uint32_t width, height, n_buckets;
    uint64_t stride;       // doubles from one plane to the next: the pixel count rounded up to even (rl_robust.hip.h)
    double* sums;          // n_buckets x 3 planes: component c of bucket j at (j * 3 + c) * stride
    uint8_t* trim;         // the last resolve's or estimate's per-pixel c, bit 7 = untrimmable: width x height bytes
    uint64_t bucket_paths[RL_ROBUST_MAX_BUCKETS]; // n[j]
    uint64_t observations; // k
    hipStream_t stream;    // clears and observes
    hipEvent_t observed;   // recorded on `stream` after an observe kernel: the plot unit's stream waits for it
    hipEvent_t ready;      // recorded on `stream` when a resolve takes the planes
    EventPair timed[2];    // around the last observe launch and the last resolve launch (rl_debug_robust_ms)
    bool timed_done[2];    // ... recorded at least once (observe), of a call that completed (resolve)
    uint32_t tiles_x, tiles_y; // the estimate's RL_ERROR_TILE tiles
    float* se;             // the estimate's per-pixel result, width x height floats
    double* tiles;         // the estimate's {t_se, t_y} per tile, tiles in raster order
    EventPair timed_estimate;  // around the last estimate launch (rl_debug_robust_estimate_ms)
    bool timed_estimate_done;  // ... recorded at least once
    Ledger ledger;
};

struct RlAdaptiveUnit {
    int device;
    uint32_t width, height, tiles_x, tiles_y;
    bool planned;              // a plan is on the device
    uint64_t n_paths;          // the plan's
    uint32_t* off;             // tiles + 1 exclusive prefix sums of the counts
    RlAdaptiveCell* cells;     // the tiles' cells
    uint32_t* weight_bits;     // the bits of w_t
    // rl_plot_unit_render_adaptive's scratch, taken at the first such call (null before it): RL_QUERY_CHUNK records each
    RlCameraSample* samples;
    RlSpectralRay* rays;
    RlPathResult* results;
    EventPair timed[3];        // around the three launches of the last chunk of the last render (rl_debug_adaptive_ms)
    bool timed_done;           // ... of a call that completed
    Ledger ledger;
};

// tests/test_adaptive_abi.py writes a stand-in handle's first fields at these offsets (the checks that read a handle before any
// device work): a field that moves must move there too.
static_assert(offsetof(RlAdaptiveUnit, width) == 4 && offsetof(RlAdaptiveUnit, height) == 8 && offsetof(RlAdaptiveUnit, planned) == 20 &&
                  offsetof(RlAdaptiveUnit, n_paths) == 24,
              "tests/test_adaptive_abi.py: test_a_stand_in_with_a_plan_is_checked_for_its_range_size_and_device");

// tests/test_robust_abi.py does the same for a robust unit, and for the device and size of the plot and gather units it is handed.
static_assert(offsetof(RlRobustUnit, width) == 4 && offsetof(RlRobustUnit, height) == 8 && offsetof(RlRobustUnit, n_buckets) == 12 &&
                  offsetof(RlRobustUnit, bucket_paths) == 40 && offsetof(RlRobustUnit, observations) == 40 + 8 * RL_ROBUST_MAX_BUCKETS &&
                  offsetof(RlPlotUnit, width) == 8 && offsetof(RlPlotUnit, height) == 12 && offsetof(RlGatherUnit, width) == 4 &&
                  offsetof(RlGatherUnit, height) == 8,
              "tests/test_robust_abi.py: test_a_stand_in_handle_is_checked_in_the_stated_order");

// tests/test_relight_abi.py does the same for a relight unit.
static_assert(offsetof(RlRelightUnit, width) == 4 && offsetof(RlRelightUnit, height) == 8 && offsetof(RlRelightUnit, n_nodes) == 12 &&
                  offsetof(RlRelightUnit, n_groups) == 16 && offsetof(RlRelightUnit, n_objects) == 20,
              "tests/test_relight_abi.py: test_a_stand_in_handle_is_checked_in_the_stated_order");

// One rank of an RCCL communicator (rl_comm_*).
struct RlComm {
    int device, rank, world;
    void* nccl; // ncclComm_t
};

namespace {

int drain_events(RlTraceUnit* u) {
    uint64_t read = 0;
    return u->timed.harvest(u->timed.pending.size(), &u->kernel_ms, &read);
}

// The instantiation of rl_trace_kernel for a launch: primitives staged in LDS or fetched from global memory, fused with
// the splat or not, an open launch or a plain one, prisms with a second bound or without.
typedef void (*TraceKernel)(const RlF4*, RlSceneLayout, RlTraceJob, RlMappedPhoton*, float*, unsigned long long*, const RlJobEntry*,
                            RlOpenDev*, RlOpenCtl*);
std::atomic<uint64_t> g_variant_launches[24]; // rl_debug_variant_launches: launches per instantiation since the library was loaded
// stage: RL_STAGE_NONE / RL_STAGE_TABLES / RL_STAGE_ALL.  Index = the four template arguments as bits -- 8: the whole scene in LDS,
// 4: fused, 2: open, 1: cylinders -- and 16 + the low three for the variants that stage the tables only.
TraceKernel trace_kernel_variant(int stage, bool fused, bool open, bool cyl) {
    const int low = (fused ? 4 : 0) | (open ? 2 : 0) | (cyl ? 1 : 0);
    const int index = stage == RL_STAGE_TABLES ? 16 + low : (stage == RL_STAGE_ALL ? 8 : 0) | low;
    g_variant_launches[index].fetch_add(1, std::memory_order_relaxed);
    static const TraceKernel table[24] = {
        rl_trace_kernel<RL_STAGE_NONE, false, false>, rl_trace_kernel<RL_STAGE_NONE, false, true>, rl_trace_kernel_open<RL_STAGE_NONE, false, false>, rl_trace_kernel_open<RL_STAGE_NONE, false, true>,
        rl_trace_kernel<RL_STAGE_NONE, true, false>, rl_trace_kernel<RL_STAGE_NONE, true, true>, rl_trace_kernel_open<RL_STAGE_NONE, true, false>, rl_trace_kernel_open<RL_STAGE_NONE, true, true>,
        rl_trace_kernel<RL_STAGE_ALL, false, false>, rl_trace_kernel<RL_STAGE_ALL, false, true>, rl_trace_kernel_open<RL_STAGE_ALL, false, false>, rl_trace_kernel_open<RL_STAGE_ALL, false, true>,
        rl_trace_kernel<RL_STAGE_ALL, true, false>, rl_trace_kernel<RL_STAGE_ALL, true, true>, rl_trace_kernel_open<RL_STAGE_ALL, true, false>, rl_trace_kernel_open<RL_STAGE_ALL, true, true>,
        rl_trace_kernel<RL_STAGE_TABLES, false, false>, rl_trace_kernel<RL_STAGE_TABLES, false, true>, rl_trace_kernel_open<RL_STAGE_TABLES, false, false>, rl_trace_kernel_open<RL_STAGE_TABLES, false, true>,
        rl_trace_kernel<RL_STAGE_TABLES, true, false>, rl_trace_kernel<RL_STAGE_TABLES, true, true>, rl_trace_kernel_open<RL_STAGE_TABLES, true, false>, rl_trace_kernel_open<RL_STAGE_TABLES, true, true>,
    };
    return table[index];
}
// The same for a unit with a wavelength table (rl_trace_unit_set_wavelengths): the WL instantiations, which take the table as one
// more argument, counted on their own (rl_debug_wavelength_variant_launches; same index).
typedef void (*TraceKernelWl)(const RlF4*, RlSceneLayout, RlTraceJob, RlMappedPhoton*, float*, unsigned long long*, const RlJobEntry*,
                              RlOpenDev*, RlOpenCtl*, const float*);
std::atomic<uint64_t> g_wavelength_variant_launches[24];
TraceKernelWl trace_kernel_variant_wl(int stage, bool fused, bool open, bool cyl) {
    const int low = (fused ? 4 : 0) | (open ? 2 : 0) | (cyl ? 1 : 0);
    const int index = stage == RL_STAGE_TABLES ? 16 + low : (stage == RL_STAGE_ALL ? 8 : 0) | low;
    g_wavelength_variant_launches[index].fetch_add(1, std::memory_order_relaxed);
    static const TraceKernelWl table[24] = {
        rl_wl_trace_kernel<RL_STAGE_NONE, false, false>, rl_wl_trace_kernel<RL_STAGE_NONE, false, true>, rl_wl_trace_open_kernel<RL_STAGE_NONE, false, false>, rl_wl_trace_open_kernel<RL_STAGE_NONE, false, true>,
        rl_wl_trace_kernel<RL_STAGE_NONE, true, false>, rl_wl_trace_kernel<RL_STAGE_NONE, true, true>, rl_wl_trace_open_kernel<RL_STAGE_NONE, true, false>, rl_wl_trace_open_kernel<RL_STAGE_NONE, true, true>,
        rl_wl_trace_kernel<RL_STAGE_ALL, false, false>, rl_wl_trace_kernel<RL_STAGE_ALL, false, true>, rl_wl_trace_open_kernel<RL_STAGE_ALL, false, false>, rl_wl_trace_open_kernel<RL_STAGE_ALL, false, true>,
        rl_wl_trace_kernel<RL_STAGE_ALL, true, false>, rl_wl_trace_kernel<RL_STAGE_ALL, true, true>, rl_wl_trace_open_kernel<RL_STAGE_ALL, true, false>, rl_wl_trace_open_kernel<RL_STAGE_ALL, true, true>,
        rl_wl_trace_kernel<RL_STAGE_TABLES, false, false>, rl_wl_trace_kernel<RL_STAGE_TABLES, false, true>, rl_wl_trace_open_kernel<RL_STAGE_TABLES, false, false>, rl_wl_trace_open_kernel<RL_STAGE_TABLES, false, true>,
        rl_wl_trace_kernel<RL_STAGE_TABLES, true, false>, rl_wl_trace_kernel<RL_STAGE_TABLES, true, true>, rl_wl_trace_open_kernel<RL_STAGE_TABLES, true, false>, rl_wl_trace_open_kernel<RL_STAGE_TABLES, true, true>,
    };
    return table[index];
}
// Ring T of rl_scan_wave: 512 bytes per wave in front of the scratch blocks, for scenes whose cull table has a third level.
size_t ring_t_bytes(const RlScene* scene) { return scene->lay.n_cluster_supers != 0u ? (size_t)(RL_TRACE_BLOCK / 64) * 512u : 0u; }
// What a launch stages in LDS beside `scratch_bytes` of per-wave scratch: the whole scene where it fits, its tables where
// those do, nothing otherwise (or when the unit was created with RL_FETCH_GLOBAL); *bytes = the staged size.
int stage_of(const RlScene* scene, int fetch, size_t scratch_bytes, size_t* bytes) {
    *bytes = 0;
    if (fetch != RL_FETCH_LDS) return RL_STAGE_NONE;
    // (what is staged is rounded up to 512 bytes: the waves' scratch behind it is 512-byte aligned, rl_trace_body)
    const size_t all = (scene->staged_bytes + 511) & ~(size_t)511, tables = (scene->tables_bytes + 511) & ~(size_t)511;
    if (scene->lay.n_cluster_supers == 0u && all + scratch_bytes <= 160 * 1024) { // (a table with a third level: the whole-scene variants do not carry its code)
        *bytes = all;
        return RL_STAGE_ALL;
    }
    if (tables + scratch_bytes <= 160 * 1024) {
        *bytes = tables;
        return RL_STAGE_TABLES;
    }
    return RL_STAGE_NONE;
}

// The argument checks the calls share (one message each).
int fetch_check(int fetch) {
    if (fetch != RL_FETCH_LDS && fetch != RL_FETCH_GLOBAL) return fail(RL_E_INVALID, "unknown fetch mode");
    return RL_OK;
}
int path_range_check(uint64_t first_path, uint64_t n) {
    if (first_path + n < first_path || first_path + n == ~0ull) return fail(RL_E_INVALID, "path indices must stay below 2^64 - 1");
    return RL_OK;
}
int max_segments_resolve(uint32_t max_segments, uint32_t* resolved) {
    if (max_segments > RL_PATH_MAX_SEGMENTS_CAP) return fail(RL_E_INVALID, "max_segments exceeds RL_PATH_MAX_SEGMENTS_CAP = 65536");
    *resolved = max_segments == 0u ? RL_PATH_MAX_SEGMENTS : max_segments;
    return RL_OK;
}

// One launch of the trace kernel on u's stream: n_paths paths from first_path on, into `photons` (un-fused) or splatted
// into plot_unit's buffer (fused).
int launch_trace(RlTraceUnit* u, const RlScene* scene, RlMappedPhoton* photons, RlPlotUnit* plot_unit, uint64_t seed,
                 uint32_t stream_id, uint64_t first_path, uint64_t n_paths) {
    if (n_paths == 0) return RL_OK;
    if (path_range_check(first_path, n_paths) != RL_OK) return RL_E_INVALID;
    float* plot = plot_unit ? plot_unit->xyz : nullptr;
    if (scene->device != u->device) return fail(RL_E_STATE, "scene and trace unit live on different devices");
    RlTraceJob job;
    job.width = u->width;
    job.height = u->height;
    job.aspect_ratio = (float)u->width / (float)u->height; // trace_unit.rs:73
    job.stream = stream_id;
    job.seed = seed;
    job.first_path = first_path;
    job.n_paths = n_paths;
    job.grace_ticks = 0;
    job.reserved = 0;
    job.wm1 = (float)(int)u->width - 1.0f;
    job.hm1 = (float)(int)u->height - 1.0f;

    // One workgroup of RL_TRACE_BLOCK threads per CU: [scene blob][per-wave scratch] in dynamic LDS.
    const size_t scratch_bytes = (RL_TRACE_BLOCK / 64) * sizeof(RlWaveScratch) + ring_t_bytes(scene);
    size_t blob_bytes = 0;
    const int stage = stage_of(scene, u->fetch, scratch_bytes, &blob_bytes);
    const bool fused = plot != nullptr;
    const bool cyl = scene->lay.prism_cylinders != 0u;
    const float* wl = u->wavelengths ? u->wavelengths->table : nullptr;
    const TraceKernel plain = wl ? nullptr : trace_kernel_variant(stage, fused, false, cyl);
    const TraceKernelWl sampled = wl ? trace_kernel_variant_wl(stage, fused, false, cyl) : nullptr;
    const void* kernel = wl ? (const void*)sampled : (const void*)plain;
    const size_t dyn = scratch_bytes + blob_bytes;
    if (u->tuned_per_cu == 0 || u->tuned_dyn != dyn || u->tuned_kernel != kernel) { // once per (unit, scene size, variant)
        // The limit is a property of the function, shared by every unit: always raise it to the whole LDS.
        RL_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        int per_cu = 1;
        RL_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, RL_TRACE_BLOCK, dyn));
        u->tuned_per_cu = per_cu < 1 ? 1 : per_cu;
        if (getenv("RL_DEBUG_LAUNCH")) fprintf(stderr, "rl: trace launch: %d workgroup(s) of %d threads per CU, %zu bytes of LDS each, stage %d\n", per_cu, RL_TRACE_BLOCK, dyn, stage);
        u->tuned_dyn = dyn;
        u->tuned_kernel = kernel; // (the instantiation itself, not some of its template arguments -- `cyl` was not among them)
    }
    uint64_t blocks = (uint64_t)u->cu_count * (uint64_t)u->tuned_per_cu;
    const uint64_t needed = (n_paths + RL_TRACE_BLOCK - 1) / RL_TRACE_BLOCK;
    if (blocks > needed) blocks = needed;

    EventPair ep;
    int rc = u->timed.take(&u->ledger, &ep);
    if (rc != RL_OK) return rc;
    rc = [&]() -> int {
        if (plot_unit) {
            RL_HIP(hipStreamWaitEvent(u->stream, plot_unit->cleared, 0)); // the splat must not race the last gather's clear
            // nor anything queued on the plot unit's own stream since (rl_plot_unit_add, the RCCL reduce, an upload)
            const int r = hand_over(plot_unit->tail, plot_unit->stream, u->stream);
            if (r != RL_OK) return r;
        }
        RL_HIP(hipMemsetAsync(u->queue, 0, sizeof(unsigned long long), u->stream));
        return timed_launch(ep, u->stream, &u->launches, [&] {
            if (wl)
                hipLaunchKernelGGL(sampled, dim3((unsigned)blocks), dim3(RL_TRACE_BLOCK), dyn, u->stream, scene->blob, scene->lay, job, photons,
                                   plot, u->queue, (const RlJobEntry*)nullptr, (RlOpenDev*)nullptr, (RlOpenCtl*)nullptr, wl);
            else
                hipLaunchKernelGGL(plain, dim3((unsigned)blocks), dim3(RL_TRACE_BLOCK), dyn, u->stream, scene->blob, scene->lay, job, photons,
                                   plot, u->queue, (const RlJobEntry*)nullptr, (RlOpenDev*)nullptr, (RlOpenCtl*)nullptr);
        });
    }();
    if (rc != RL_OK) {
        u->timed.give_back(ep); // (whatever of it was recorded is recorded again by the launch that takes it next)
        return rc;
    }
    u->timed.pending.push_back(ep);
    // `rendered`: everything that fills this unit's photons so far.  A fused launch: the plot stream's tail covers this splat.
    if (plot_unit) rc = hand_over(u->rendered, u->stream, plot_unit->stream);
    else RL_HIP(hipEventRecord(u->rendered, u->stream));
    if (rc != RL_OK) return rc;
    if (u->timed.pending.size() > 512) return drain_events(u);
    return RL_OK;
}

// ---- the persistent ray kernels beside the trace kernel (rl_query.hip.h, rl_occlusion.hip.h, rl_paths.hip.h, rl_step.hip.h, rl_path_list.hip.h) ----
// A family is one kernel template's six instantiations, index = 2 * stage + cylinders, and the launches of each since the library
// was loaded (rl_debug_{query,occlusion,path,film,step,path_list,light,light_film,direct,feature}_launches).  P: the kernel's parameters behind the scene blob and its layout.
template <class... P>
struct KernelFamily {
    void (*variants[6])(const RlF4*, RlSceneLayout, P...);
    std::atomic<uint64_t> launches[6];
};
#define RL_VARIANTS(K) {{K<RL_STAGE_NONE, false>, K<RL_STAGE_NONE, true>, K<RL_STAGE_TABLES, false>, K<RL_STAGE_TABLES, true>, K<RL_STAGE_ALL, false>, K<RL_STAGE_ALL, true>}, {}}
KernelFamily<const RlRay*, RlRayHit*, uint32_t> g_query_kernels = RL_VARIANTS(rl_query_kernel);
KernelFamily<const RlRay*, uint8_t*, uint32_t> g_occlusion_kernels = RL_VARIANTS(rl_occlusion_kernel);
KernelFamily<const RlSpectralRay*, RlPathResult*, uint32_t, uint64_t, uint32_t, uint64_t, uint32_t, unsigned long long*> g_path_kernels = RL_VARIANTS(rl_ray_paths_kernel);
KernelFamily<const RlCameraSample*, RlPathResult*, uint32_t, uint64_t, uint32_t, uint64_t, uint32_t, unsigned long long*> g_film_kernels = RL_VARIANTS(rl_film_paths_kernel);
KernelFamily<RlPathState*, RlRayHit*, uint32_t, uint64_t, uint32_t, uint32_t, unsigned long long*> g_step_kernels = RL_VARIANTS(rl_step_kernel);
KernelFamily<RlPathState*, RlRayHit*, unsigned long long*> g_list_step_kernels = RL_VARIANTS(rl_list_step_kernel);
KernelFamily<unsigned long long*> g_light_kernels = RL_VARIANTS(rl_light_kernel);
KernelFamily<unsigned long long*> g_light_film_kernels = RL_VARIANTS(rl_light_film_kernel);
KernelFamily<unsigned long long*> g_direct_kernels = RL_VARIANTS(rl_direct_paths_kernel);
KernelFamily<unsigned long long*> g_feature_kernels = RL_VARIANTS(rl_feature_paths_kernel);
#undef RL_VARIANTS
template <class... P>
int family_launches(const KernelFamily<P...>& family, uint64_t* out) {
    if (!out) return fail(RL_E_INVALID, "null output");
    for (int k = 0; k < 6; ++k) out[k] = family.launches[k].load(std::memory_order_relaxed);
    return RL_OK;
}

// What a query call runs on: a stream of its own and, for the host path, device buffers of RL_QUERY_CHUNK records.
// Each device keeps the contexts of finished calls for the next ones, so concurrent callers never share a stream or a buffer
// and a steady caller allocates nothing.
#define RL_QUERY_CHUNK (1u << 20)
// The path, film and step calls run on the same contexts: 32-byte records (rays, spectral rays, photons; the film's results) go
// through STAGING_RAYS, 48-byte ones (hits, camera samples; the path results) through STAGING_HITS, path states through STAGING_STATES.
enum { STAGING_RAYS, STAGING_HITS, STAGING_STATES, STAGING_COUNT };
const size_t staging_record_bytes[STAGING_COUNT] = {sizeof(RlRay), sizeof(RlRayHit), sizeof(RlPathState)};
// A device buffer that is grown on demand and never shrunk (device_reserve).
struct GrowBuffer {
    void* p = nullptr;
    size_t bytes = 0;
};
struct QueryCtx {
    hipStream_t stream = nullptr;
    void* staging[STAGING_COUNT] = {};   // host path only (allocated on first use, RL_QUERY_CHUNK records each)
    unsigned long long* queue = nullptr; // path, film and step calls only (allocated on first use): the counter of an RlFilmQueue
    GrowBuffer pack;                     // rl_scene_step_path_list* only: the compaction's counts and survivors (launch_list_step)
    GrowBuffer direct;                   // rl_plot_unit_render_samples_direct* only: the loop's working buffers (direct_chunk)
};
// What a call's helpers run on: a query context borrowed for the call, the stream that every copy and launch of the call goes on
// (the context's own for a scene call, the plot unit's for a film call) and the device's CU count.
struct CallCtx {
    QueryCtx* q;
    hipStream_t stream;
    int cus;
};
static_assert(sizeof(RlSpectralRay) == sizeof(RlRay) && sizeof(RlMappedPhoton) <= sizeof(RlRay) && sizeof(RlCameraSample) == sizeof(RlRayHit) &&
                  sizeof(RlPathResult) <= sizeof(RlRay),
              "the path and film calls stage their records through a query context's buffers");
struct DeviceQueries {
    std::mutex lock;
    std::vector<QueryCtx*> idle;
    // resident workgroups per CU of each persistent kernel launched so far, for the dynamic LDS size last seen: by the kernel's address
    std::map<const void*, std::pair<size_t, int>> resident;
};
DeviceQueries* queries_of(int device) {
    static DeviceQueries all[64];
    return &all[device >= 0 && device < 64 ? device : 0];
}
int query_ctx_acquire(int device, QueryCtx** out) { // device current
    DeviceQueries* d = queries_of(device);
    {
        std::lock_guard<std::mutex> guard(d->lock);
        if (!d->idle.empty()) {
            *out = d->idle.back();
            d->idle.pop_back();
            return RL_OK;
        }
    }
    QueryCtx* q = new (std::nothrow) QueryCtx();
    if (!q) return fail(RL_E_INVALID, "out of host memory");
    const hipError_t e = hipStreamCreateWithFlags(&q->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete q;
        return fail(RL_E_HIP, std::string("query stream: ") + hipGetErrorString(e));
    }
    *out = q;
    return RL_OK;
}
void query_ctx_release(int device, QueryCtx* q) {
    DeviceQueries* d = queries_of(device);
    std::lock_guard<std::mutex> guard(d->lock);
    d->idle.push_back(q);
}
// The context's queue counter (an RlFilmQueue, an RlPathListQueue, an RlLightQueue, an RlLightFilmQueue, an RlDirectQueue or an RlFeatureQueue: a launch's constants sit behind it), allocated on first use.
int query_ctx_queue(QueryCtx* q) {
    const size_t bytes = std::max({sizeof(RlFilmQueue), sizeof(RlPathListQueue), sizeof(RlLightQueue), sizeof(RlLightFilmQueue), sizeof(RlDirectQueue), sizeof(RlFeatureQueue)});
    if (!q->queue) RL_HIP(hipMalloc((void**)&q->queue, bytes));
    return RL_OK;
}

// Room for `bytes` in one of a context's scratch buffers.  (Nothing that uses the buffer runs.)
int device_reserve(GrowBuffer* b, size_t bytes) {
    if (b->bytes >= bytes) return RL_OK;
    if (b->p) RL_HIP(hipFree(b->p));
    b->p = nullptr;
    b->bytes = 0;
    RL_HIP(hipMalloc(&b->p, bytes));
    b->bytes = bytes;
    return RL_OK;
}

// Resident workgroups per CU of a persistent kernel with `dyn` bytes of dynamic LDS.
int resident_per_cu(int device, const void* kernel, size_t dyn, int* out) {
    DeviceQueries* d = queries_of(device);
    std::lock_guard<std::mutex> guard(d->lock);
    std::pair<size_t, int>& slot = d->resident[kernel];
    if (slot.second == 0 || slot.first != dyn) {
        RL_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        int k = 1;
        RL_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&k, kernel, RL_TRACE_BLOCK, dyn));
        slot = {dyn, k < 1 ? 1 : k};
    }
    *out = slot.second;
    return RL_OK;
}

// One launch of a family's kernel on c's stream for n (> 0) records of device arrays: the instantiation for what the scene stages
// and how its prisms are bound, as many workgroups as stay resident (or as the records need), args... behind the blob and the layout.
// What a family's queue needs before the launch is the caller's.
template <class... P, class... A>
int launch_persistent(const CallCtx& c, KernelFamily<P...>& family, const RlScene* scene, int fetch, uint32_t n, A... args) {
    const size_t scratch_bytes = (RL_TRACE_BLOCK / 64) * sizeof(RlWaveScratch) + ring_t_bytes(scene);
    size_t blob_bytes = 0;
    const int stage = stage_of(scene, fetch, scratch_bytes, &blob_bytes);
    const int index = 2 * stage + (scene->lay.prism_cylinders != 0u ? 1 : 0);
    family.launches[index].fetch_add(1, std::memory_order_relaxed);
    auto kernel = family.variants[index];
    const size_t dyn = scratch_bytes + blob_bytes;
    int per_cu = 0;
    const int rc = resident_per_cu(scene->device, (const void*)kernel, dyn, &per_cu);
    if (rc != RL_OK) return rc;
    uint64_t blocks = (uint64_t)c.cus * (uint64_t)per_cu;
    const uint64_t needed = ((uint64_t)n + RL_TRACE_BLOCK - 1) / RL_TRACE_BLOCK;
    if (blocks > needed) blocks = needed;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(RL_TRACE_BLOCK), dyn, c.stream, scene->blob, scene->lay, args...);
    RL_HIP(hipGetLastError());
    return RL_OK;
}

// One array of a host-staged call: the caller's records, which of the context's buffers they go through, and which way.
struct Staged {
    int slot;
    void* host; // (null: the call does without this array)
    size_t record_bytes;
    bool in, out;
};
Staged staged_in(int slot, const void* host, size_t record_bytes) { return Staged{slot, const_cast<void*>(host), record_bytes, true, false}; }
Staged staged_out(int slot, void* host, size_t record_bytes) { return Staged{slot, host, record_bytes, false, true}; }
Staged staged_inout(int slot, void* host, size_t record_bytes) { return Staged{slot, host, record_bytes, true, true}; }
// The host forms: records [0, n) in chunks of RL_QUERY_CHUNK through the context's staging buffers (allocated here on first use) --
// copy in, launch(first, k) for records [first, first + k), copy out, synchronise (the next chunk overwrites the buffers).
template <class N, class Launch>
int staged_chunks(const CallCtx& c, N n, std::initializer_list<Staged> arrays, Launch launch) {
    for (const Staged& a : arrays)
        if (a.host && !c.q->staging[a.slot]) RL_HIP(hipMalloc(&c.q->staging[a.slot], (size_t)RL_QUERY_CHUNK * staging_record_bytes[a.slot]));
    for (N first = 0; first < n;) {
        const N k = n - first < RL_QUERY_CHUNK ? n - first : (N)RL_QUERY_CHUNK;
        for (const Staged& a : arrays)
            if (a.host && a.in)
                RL_HIP(hipMemcpyAsync(c.q->staging[a.slot], (const char*)a.host + (size_t)first * a.record_bytes, (size_t)k * a.record_bytes, hipMemcpyHostToDevice, c.stream));
        const int r = launch(first, k);
        if (r != RL_OK) return r;
        for (const Staged& a : arrays)
            if (a.host && a.out)
                RL_HIP(hipMemcpyAsync((char*)a.host + (size_t)first * a.record_bytes, c.q->staging[a.slot], (size_t)k * a.record_bytes, hipMemcpyDeviceToHost, c.stream));
        RL_HIP(hipStreamSynchronize(c.stream));
        first += k;
    }
    return RL_OK;
}

// One array of a whole-array host call: the caller's records (null: the call does without this array), their size, which way
// run() copies them, and the call's own device buffer for them (null: not given, or empty).
struct Whole {
    void* host;
    size_t bytes;
    bool in, out;
    void* dev = nullptr;
};
Whole whole_in(const void* host, size_t bytes) { return Whole{const_cast<void*>(host), bytes, true, false}; }
Whole whole_inout(void* host, size_t bytes) { return Whole{host, bytes, true, true}; }
Whole whole_scratch(void* host, size_t bytes) { return Whole{host, bytes, false, false}; } // (the caller copies what it needs of it)
// The host forms that are not chunked (the context's staging buffers hold 2^20 records, and a list names states anywhere in the
// array): device buffers of the call's own for the whole arrays, freed on every way out.  The arrays are the caller's named ones.
struct WholeArrays {
    Whole* arrays[6] = {};
    template <class... W>
    explicit WholeArrays(W*... w) : arrays{w...} {}
    WholeArrays(const WholeArrays&) = delete;
    ~WholeArrays() {
        for (Whole* a : arrays)
            if (a && a->dev) (void)hipFree(a->dev);
    }
    int allocate() {
        for (Whole* a : arrays)
            if (a && a->host && a->bytes) RL_HIP(hipMalloc(&a->dev, a->bytes));
        return RL_OK;
    }
    // On `stream`: the copies in, launch(), the copies out.  Not synchronised.
    template <class Launch>
    int run(hipStream_t stream, Launch launch) {
        for (Whole* a : arrays)
            if (a && a->dev && a->in) RL_HIP(hipMemcpyAsync(a->dev, a->host, a->bytes, hipMemcpyHostToDevice, stream));
        const int r = launch();
        if (r != RL_OK) return r;
        for (Whole* a : arrays)
            if (a && a->dev && a->out) RL_HIP(hipMemcpyAsync(a->host, a->dev, a->bytes, hipMemcpyDeviceToHost, stream));
        return RL_OK;
    }
};

int query_check(const RlScene* scene, int fetch, const void* rays, uint32_t n_rays, const void* hits) {
    if (fetch_check(fetch) != RL_OK) return RL_E_INVALID;
    if (n_rays > 0 && (!rays || !hits)) return fail(RL_E_INVALID, "null ray or hit buffer");
    if (!scene) return fail(RL_E_INVALID, "null scene");
    return RL_OK;
}

// The arrays of a _device call, in the order they are checked (null: the call does without that one), and the names its messages
// use: the entry point and its form for host arrays.  A host form has none.
struct DeviceArrays {
    const char* what = nullptr;
    const char* host_form = nullptr;
    const void* pointers[6] = {};
};
// Every array of a _device call must be memory the owner's device can address: a pageable host pointer there would fault the
// device.  Accepted: device memory of that device, managed memory, and pinned host memory mapped at the same address.  (The
// runtime reports pageable host memory as hipMemoryTypeUnregistered, or fails.)
int device_buffers_check(int device, const char* owner, const DeviceArrays& arrays) {
    for (const void* p : arrays.pointers) {
        if (!p) continue;
        hipPointerAttribute_t attr;
        std::memset(&attr, 0, sizeof attr);
        if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
            (void)hipGetLastError();
            attr.type = hipMemoryTypeUnregistered;
        }
        const bool ok = (attr.type == hipMemoryTypeDevice && attr.device == device) || attr.type == hipMemoryTypeManaged ||
                        (attr.type == hipMemoryTypeHost && attr.devicePointer == p);
        if (!ok)
            return fail(RL_E_INVALID, std::string(arrays.what) + ": a buffer is not device memory of the " + owner + "'s device (host arrays: " +
                                          arrays.host_form + ")");
    }
    return RL_OK;
}
// The alignment a _device call asks of its arrays: `which` names the one (or the ones, their addresses or-ed) in the message.
int aligned_check(const char* what, const char* which, unsigned alignment, std::initializer_list<const void*> pointers) {
    uintptr_t bits = 0;
    for (const void* p : pointers) bits |= (uintptr_t)p;
    if ((bits & (alignment - 1u)) == 0) return RL_OK;
    return fail(RL_E_INVALID, std::string(what) + ": " + which + " is not " + std::to_string(alignment) + "-byte aligned");
}
int states_aligned(const void* states, const char* what) { return aligned_check(what, "the state buffer", 16, {states}); }
// A null list names states 0 .. n_list - 1.
int identity_list_check(const void* list, uint32_t n_list, uint32_t n_states) {
    if (!list && n_list > n_states) return fail(RL_E_INVALID, "the identity list (list = NULL) is longer than the state buffer");
    return RL_OK;
}

// ---- caller-supplied paths (rl_scene_camera_rays*, rl_scene_render_rays*, rl_paths.hip.h) -----------------------------------
struct PathJob {
    uint64_t seed;
    uint32_t stream;
    uint32_t max_segments; // resolved: 1 .. RL_PATH_MAX_SEGMENTS_CAP
};

// rays [0, n) of device arrays as paths first_path .. first_path + n - 1 (n > 0): one launch of the path kernel on c's stream,
// behind the zeroing of its queue.
int launch_paths(const CallCtx& c, const RlScene* scene, int fetch, const PathJob& job, uint64_t first_path, const RlSpectralRay* rays,
                 RlPathResult* results, uint32_t n) {
    const int rc = query_ctx_queue(c.q);
    if (rc != RL_OK) return rc;
    RL_HIP(hipMemsetAsync(c.q->queue, 0, sizeof(unsigned long long), c.stream));
    return launch_persistent(c, g_path_kernels, scene, fetch, n, rays, results, n, job.seed, job.stream, first_path, job.max_segments, c.q->queue);
}

unsigned grid_for(uint64_t work_items, int cu_count);

// The camera kernel for paths first_path .. first_path + n - 1 into device array `samples` (n > 0), on c's stream.
int launch_camera(const CallCtx& c, const RlScene* scene, uint32_t width, uint32_t height, uint64_t seed, uint32_t stream, uint64_t first_path,
                  RlCameraSample* samples, uint32_t n) {
    const float aspect_ratio = (float)width / (float)height; // trace_unit.rs:73, as launch_trace has it
    hipLaunchKernelGGL(rl_camera_rays_kernel, dim3(grid_for(n, c.cus)), dim3(RL_BLOCK), 0, c.stream, scene->blob, scene->lay, aspect_ratio,
                       seed, stream, first_path, samples, n);
    RL_HIP(hipGetLastError());
    return RL_OK;
}

int paths_check(const RlScene* scene, int fetch, const void* rays, uint32_t n_rays, const void* results, uint64_t first_path,
                uint32_t max_segments, PathJob* job) {
    if (fetch_check(fetch) != RL_OK) return RL_E_INVALID;
    if (n_rays > 0 && (!rays || !results)) return fail(RL_E_INVALID, "null ray or result buffer");
    int rc = query_check(scene, fetch, rays, n_rays, results);
    if (rc != RL_OK) return rc;
    if ((rc = max_segments_resolve(max_segments, &job->max_segments)) != RL_OK) return rc;
    return path_range_check(first_path, n_rays);
}

int camera_check(const RlScene* scene, uint32_t width, uint32_t height, uint64_t first_path, uint32_t n, const void* samples) {
    if (!scene) return fail(RL_E_INVALID, "null scene");
    if (n > 0 && !samples) return fail(RL_E_INVALID, "null sample buffer");
    if (width == 0 || height == 0) return fail(RL_E_INVALID, "camera rays: zero image size");
    if (check_image_size("camera rays", width, height) != RL_OK) return RL_E_INVALID;
    return path_range_check(first_path, n);
}

unsigned grid_for(uint64_t work_items, int cu_count) {
    uint64_t blocks = (work_items + RL_BLOCK - 1) / RL_BLOCK;
    const uint64_t cap = (uint64_t)cu_count * 8;
    if (blocks > cap) blocks = cap;
    if (blocks < 1) blocks = 1;
    return (unsigned)blocks;
}

int cu_count_of(int device, int* out) {
    // hipGetDeviceProperties is slow; the answer never changes, so remember it per device.
    static std::mutex lock;
    static int cached[64];
    if (device >= 0 && device < 64) {
        std::lock_guard<std::mutex> guard(lock);
        if (cached[device] > 0) {
            *out = cached[device];
            return RL_OK;
        }
    }
    hipDeviceProp_t prop;
    RL_HIP(hipGetDeviceProperties(&prop, device));
    *out = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (device >= 0 && device < 64) {
        std::lock_guard<std::mutex> guard(lock);
        cached[device] = *out;
    }
    return RL_OK;
}

int plot_settle(RlPlotUnit* plot);

// Runs body(c) on `device` with a query context borrowed, and returns when the call's stream has drained (also after a failure:
// nothing of the call may still run when the context's buffers are handed on).  The stream is the context's own, or that of the
// plot unit `film`, whose tail is every write into its buffer so far: a render begun into that unit ends first.  A _device form's
// arrays are checked once the device is current.
template <class Body>
int with_call_ctx(int device, const char* owner, RlPlotUnit* film, const DeviceArrays& arrays, Body body) {
    int cus = 256;
    int rc = enter_device(device, &cus);
    if (rc != RL_OK) return rc;
    if ((rc = device_buffers_check(device, owner, arrays)) != RL_OK) return rc;
    if (film && (rc = plot_settle(film)) != RL_OK) return rc;
    QueryCtx* q = nullptr;
    if ((rc = query_ctx_acquire(device, &q)) != RL_OK) return rc;
    const CallCtx c{q, film ? film->stream : q->stream, cus};
    rc = drained(c.stream, body(c));
    query_ctx_release(device, q);
    return rc;
}
// A scene call: on a stream of the call's own.  A host form has no arrays to check.
template <class Body>
int with_query_ctx(const RlScene* scene, const DeviceArrays& arrays, Body body) {
    return with_call_ctx(scene->device, "scene", nullptr, arrays, body);
}
template <class Body>
int with_query_ctx(const RlScene* scene, Body body) { return with_query_ctx(scene, DeviceArrays{}, body); }
// A film call: everything is queued on the plot unit's stream; the context lends its buffers and its queue counter, and its own
// stream stays idle.
template <class Body>
int with_film_ctx(RlPlotUnit* u, const DeviceArrays& arrays, Body body) {
    return with_call_ctx(u->device, "plot unit", u, arrays, body);
}
template <class Body>
int with_film_ctx(RlPlotUnit* u, Body body) { return with_film_ctx(u, DeviceArrays{}, body); }

// ---- caller-held path states (rl_scene_begin_paths*, rl_scene_step_paths*, rl_step.hip.h) -----------------------------------
// One segment for the live states of device array states [0, n) (n > 0): one launch of the step kernel on c's stream, behind the
// zeroing of its chunk counter.  `hits` may be null.
int launch_step(const CallCtx& c, const RlScene* scene, int fetch, uint64_t seed, uint32_t stream, uint32_t flags, RlPathState* states,
                RlRayHit* hits, uint32_t n) {
    const int rc = query_ctx_queue(c.q);
    if (rc != RL_OK) return rc;
    RL_HIP(hipMemsetAsync(c.q->queue, 0, sizeof(unsigned long long), c.stream));
    return launch_persistent(c, g_step_kernels, scene, fetch, n, states, hits, n, seed, stream, flags, c.q->queue);
}

// One segment for the states of device array states [0, n_states) that device array list [0, n_list) names (n_list > 0; a null
// list: states 0 .. n_list - 1), then the indices of the listed states that are still live to device array live_list, in the
// list's order, and their number to host word *n_live when c's stream is next synchronised.  hits, live_list and n_live may be
// null; live_list may be list.  On c's stream: the copy that zeroes the chunk counter and writes the list's block behind it
// (RlPathListQueue), the list-step kernel and, when live_list or n_live is given, the scan of the chunks' counts, the pack into live_list and the 4-byte copy of the last running total.  The
// scratch of the compaction is the context's: one count per chunk of 64 list positions, then one survivor slot per list position.
int launch_list_step(const CallCtx& c, const RlScene* scene, int fetch, uint64_t seed, uint32_t stream, uint32_t flags, RlPathState* states,
                     uint32_t n_states, const uint32_t* list, uint32_t n_list, RlRayHit* hits, uint32_t* live_list, uint32_t* n_live) {
    QueryCtx* q = c.q;
    int rc = query_ctx_queue(q);
    if (rc != RL_OK) return rc;
    const uint32_t n_chunks = (uint32_t)(((uint64_t)n_list + 63u) / 64u);
    uint32_t *counts = nullptr, *survivors = nullptr;
    if (live_list || n_live) {
        if ((rc = device_reserve(&q->pack, ((size_t)n_chunks + n_list) * sizeof(uint32_t))) != RL_OK) return rc;
        counts = (uint32_t*)q->pack.p;
        survivors = counts + n_chunks;
    }
    RlPathListQueue lq;
    lq.next = 0;
    lq.job.list = list;
    lq.job.survivors = survivors;
    lq.job.n_list = n_list;
    lq.job.n_states = n_states;
    lq.job.seed = seed;
    lq.job.stream = stream;
    lq.job.flags = flags;
    // (from pageable memory: the copy has left `lq` when the call returns)
    RL_HIP(hipMemcpyAsync(q->queue, &lq, sizeof lq, hipMemcpyHostToDevice, c.stream));
    rc = launch_persistent(c, g_list_step_kernels, scene, fetch, n_list, states, hits, q->queue);
    if (rc != RL_OK || !counts) return rc;
    hipLaunchKernelGGL(rl_list_scan_kernel, dim3(1), dim3(RL_LIST_SCAN_BLOCK), 0, c.stream, counts, n_chunks);
    RL_HIP(hipGetLastError());
    if (live_list) {
        hipLaunchKernelGGL(rl_list_pack_kernel, dim3(grid_for((uint64_t)n_chunks * 64u, c.cus)), dim3(RL_BLOCK), 0, c.stream, (const uint32_t*)counts,
                           (const uint32_t*)survivors, n_chunks, live_list);
        RL_HIP(hipGetLastError());
    }
    if (n_live) RL_HIP(hipMemcpyAsync(n_live, counts + (n_chunks - 1u), sizeof(uint32_t), hipMemcpyDeviceToHost, c.stream));
    return RL_OK;
}

// The words of a light launch's block that rl_light_kernel and rl_light_film_kernel share (`samples` may be null for the second).
RlLightJob light_job(const RlScene* scene, uint64_t seed, uint32_t stream, const RlPathState* states, uint32_t n_states, const uint32_t* list,
                     uint32_t n_list, const RlRayHit* hits, RlLightSample* samples) {
    RlLightJob job;
    std::memset(&job, 0, sizeof job);
    job.states = states;
    job.hits = hits;
    job.list = list;
    job.emitters = scene->emitters;
    job.samples = samples;
    job.n_list = n_list;
    job.n_states = n_states;
    job.n_emitters = (uint32_t)scene->emitter_objects.size();
    job.stream = stream;
    job.seed = seed;
    return job;
}

// One direct-light sample for the states of device array states [0, n_states) that device array list [0, n_list) names (n_list > 0;
// a null list: states 0 .. n_list - 1), from device array hits into device array samples, both indexed by state.  On c's stream: the
// copy that zeroes the chunk counter and writes the launch's block behind it (RlLightQueue), then the light kernel.
int launch_light(const CallCtx& c, const RlScene* scene, int fetch, uint64_t seed, uint32_t stream, const RlPathState* states, uint32_t n_states,
                 const uint32_t* list, uint32_t n_list, const RlRayHit* hits, RlLightSample* samples) {
    const int rc = query_ctx_queue(c.q);
    if (rc != RL_OK) return rc;
    RlLightQueue lq;
    std::memset(&lq, 0, sizeof lq);
    lq.job = light_job(scene, seed, stream, states, n_states, list, n_list, hits, samples);
    // (from pageable memory: the copy has left `lq` when the call returns)
    RL_HIP(hipMemcpyAsync(c.q->queue, &lq, sizeof lq, hipMemcpyHostToDevice, c.stream));
    return launch_persistent(c, g_light_kernels, scene, fetch, n_list, c.q->queue);
}

int light_check(const RlScene* scene, int fetch, const void* states, uint32_t n_states, const void* list, uint32_t n_list, const void* hits,
                const void* samples) {
    if (fetch_check(fetch) != RL_OK) return RL_E_INVALID;
    if (n_list > 0 && (!states || !hits || !samples)) return fail(RL_E_INVALID, "null state, hit or sample buffer");
    if (!scene) return fail(RL_E_INVALID, "null scene");
    return identity_list_check(list, n_list, n_states);
}

// The sampleable emitters of a description, in scan order (include/robigo_luculenta.h: rl_scene_emitters): their table as
// rl_light_sample reads it (rl_core.h, RL_EMITTER_STRIDE records each) and their object indices.
void emitter_table(const RlObjectDesc* objects, uint32_t n_objects, std::vector<RlF4>* table, std::vector<uint32_t>* indices) {
    table->clear();
    indices->clear();
    for (uint32_t i = 0; i < n_objects; ++i) {
        const RlObjectDesc& o = objects[i];
        if (o.material_kind != RL_MATERIAL_BLACK_BODY) continue;
        const bool bounded = o.f0 > 0.0f && o.f0 < INFINITY; // (false for NaN)
        const float n2 = o.v0.x * o.v0.x + o.v0.y * o.v0.y + o.v0.z * o.v0.z;
        RlF4 a, b, c;
        if (o.surface_kind == RL_SURFACE_SPHERE && bounded) {
            a = RlF4{o.v0.x, o.v0.y, o.v0.z, o.f0};
            b = RlF4{0.0f, 0.0f, 0.0f, rl_u2f((uint32_t)RL_SURFACE_SPHERE)};
        } else if (o.surface_kind == RL_SURFACE_CIRCLE && bounded && fabsf(n2 - 1.0f) <= 0x1p-20f) {
            a = RlF4{o.v1.x, o.v1.y, o.v1.z, o.f0};
            b = RlF4{o.v0.x, o.v0.y, o.v0.z, rl_u2f((uint32_t)RL_SURFACE_CIRCLE)};
        } else {
            continue;
        }
        c = RlF4{o.m0, rl_black_body_normalisation(o.m0, o.m1), rl_u2f(i), 0.0f}; // (the factor rl_flatten_scene gives the object record)
        table->push_back(a);
        table->push_back(b);
        table->push_back(c);
        indices->push_back(i);
    }
}

// The begin kernel for device arrays rays, states [0, n) (n > 0) as paths first_path .. first_path + n - 1, on c's stream.
int launch_begin(const CallCtx& c, uint64_t first_path, const RlSpectralRay* rays, RlPathState* states, uint32_t n) {
    hipLaunchKernelGGL(rl_begin_paths_kernel, dim3(grid_for(n, c.cus)), dim3(RL_BLOCK), 0, c.stream, rays, first_path, states, n);
    RL_HIP(hipGetLastError());
    return RL_OK;
}

int step_check(const RlScene* scene, int fetch, uint32_t flags, const void* states, uint32_t n) {
    if (fetch_check(fetch) != RL_OK) return RL_E_INVALID;
    if (flags & ~(uint32_t)RL_STEP_NO_ROULETTE) return fail(RL_E_INVALID, "unknown step flag");
    if (n > 0 && !states) return fail(RL_E_INVALID, "null state buffer");
    if (!scene) return fail(RL_E_INVALID, "null scene");
    return RL_OK;
}

int path_list_check(const RlScene* scene, int fetch, uint32_t flags, const void* states, uint32_t n_states, const void* list, uint32_t n_list) {
    const int rc = step_check(scene, fetch, flags, states, n_list);
    return rc != RL_OK ? rc : identity_list_check(list, n_list, n_states);
}

int begin_check(const RlScene* scene, uint64_t first_path, const void* rays, uint32_t n, const void* states) {
    if (n > 0 && (!rays || !states)) return fail(RL_E_INVALID, "null ray or state buffer");
    if (!scene) return fail(RL_E_INVALID, "null scene");
    return path_range_check(first_path, n);
}

} // namespace

extern "C" {

const char* rl_last_error(void) { return g_error.c_str(); }

int rl_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int rl_device_pci_bus_id(int device, char* out, uint32_t cap) {
    if (!out || cap < 16) return fail(RL_E_INVALID, "output buffer too small for a PCI bus id");
    const int rc = use_device(device);
    if (rc != RL_OK) return rc;
    RL_HIP(hipDeviceGetPCIBusId(out, (int)cap, device));
    return RL_OK;
}

const char* rl_version(void) { return "robigo-luculenta_amd 0.3 (gfx950)"; }

#ifndef RL_BUILD_ID
#define RL_BUILD_ID "unknown"
#endif
const char* rl_build_id(void) { return RL_BUILD_ID; }

// ---- scene --------------------------------------------------------------------------------------

int rl_scene_builtin_desc(int which, int param, RlObjectDesc* objects, uint32_t cap, uint32_t* n_objects,
                          RlCameraDesc* camera) {
    std::vector<RlObjectDesc> v;
    RlCameraDesc cam;
    const uint32_t n = rl_builtin_scene(which, param, &v, &cam);
    if (n == 0) return fail(RL_E_INVALID, "unknown built-in scene");
    if (n_objects) *n_objects = n;
    if (camera) *camera = cam;
    if (!objects || cap < n) return fail(RL_E_INVALID, "object array too small for the built-in scene");
    std::memcpy(objects, v.data(), n * sizeof(RlObjectDesc));
    return RL_OK;
}

int rl_scene_desc_save(const char* path, const RlSceneDesc* desc) {
    if (!path || !desc || (!desc->objects && desc->n_objects)) return fail(RL_E_INVALID, "null argument");
    FILE* f = std::fopen(path, "wb");
    if (!f) return fail(RL_E_IO, std::string("failed to open file ") + path);
    const uint32_t header[2] = {1u, desc->n_objects};
    bool ok = std::fwrite("RLSC", 1, 4, f) == 4 && std::fwrite(header, 4, 2, f) == 2 &&
              std::fwrite(&desc->camera, sizeof(RlCameraDesc), 1, f) == 1 &&
              std::fwrite(desc->objects, sizeof(RlObjectDesc), desc->n_objects, f) == desc->n_objects;
    ok = (std::fclose(f) == 0) && ok;
    return ok ? RL_OK : fail(RL_E_IO, std::string("failed to write scene file ") + path);
}

int rl_scene_desc_load(const char* path, RlObjectDesc* objects, uint32_t cap, uint32_t* n_objects, RlCameraDesc* camera) {
    if (!path) return fail(RL_E_INVALID, "null path");
    FILE* f = std::fopen(path, "rb");
    if (!f) return fail(RL_E_IO, std::string("failed to open file ") + path);
    char magic[4];
    uint32_t header[2] = {0, 0};
    RlCameraDesc cam;
    bool ok = std::fread(magic, 1, 4, f) == 4 && std::memcmp(magic, "RLSC", 4) == 0 && std::fread(header, 4, 2, f) == 2 &&
              header[0] == 1u && std::fread(&cam, sizeof cam, 1, f) == 1;
    if (!ok) {
        std::fclose(f);
        return fail(RL_E_IO, std::string("not a version-1 RLSC scene file: ") + path);
    }
    if (n_objects) *n_objects = header[1];
    if (camera) *camera = cam;
    if (!objects || cap < header[1]) {
        std::fclose(f);
        return fail(RL_E_INVALID, "object array too small for the scene file");
    }
    ok = std::fread(objects, sizeof(RlObjectDesc), header[1], f) == header[1];
    std::fclose(f);
    return ok ? RL_OK : fail(RL_E_IO, std::string("truncated scene file ") + path);
}

int rl_scene_create(const RlSceneDesc* desc, int device, RlScene** out) {
    if (!out) return fail(RL_E_INVALID, "null output handle");
    *out = nullptr;
    RlFlatScene fs;
    const char* err = "";
    int rc = rl_flatten_scene(desc, &fs, &err);
    if (rc != RL_OK) return fail(rc, err);
    if ((rc = use_device(device)) != RL_OK) return rc;

    // One blob: spheres || planes | parabs | prisms | cull table | prism cylinders | camera || objects | cie | sphere_obj | sphere_r2 (padded to 16 B).
    std::vector<RlF4> blob;
    RlSceneLayout lay;
    std::memset(&lay, 0, sizeof lay);
    auto append = [&](const std::vector<RlF4>& v) {
        const uint32_t off = (uint32_t)blob.size();
        blob.insert(blob.end(), v.begin(), v.end());
        return off;
    };
    append(fs.spheres);
    for (size_t pos = fs.cluster_base; pos < fs.spheres.size(); ++pos) blob[pos].w = fs.sphere_cull_w[pos]; // see RlSceneView::sphere_r2
    // the tables (RlSceneLayout: records [off_planes, off_objects)) ...
    lay.off_planes = append(fs.planes);
    lay.off_parabs = append(fs.parabs);
    lay.off_prisms = append(fs.prisms);
    lay.off_cull = append(fs.cull_bounds);
    lay.off_prism_cyl = append(fs.prism_cyl);
    lay.prism_cylinders = fs.prism_cylinders ? 1u : 0u;
    lay.group_gc = fs.group_gc;
    lay.small_ordered = (fs.small_ordered ? 1u : 0u) | (fs.small_axis_z ? 2u : 0u); // (bit 1: rl_scan_wave, the six small primitives of the built-in room)
    lay.off_camera = append(fs.camera_rec);
    lay.cull_cmax2 = fs.cull_cmax2;
    // ... then the per-object arrays
    lay.off_objects = append(fs.objects);
    // (an object's group bits hold 26 bits -- a blob index on the device -- and rl_object_bits masks silently)
    if (blob.size() >= (1u << 26) || fs.cluster_base + fs.spheres.size() >= (1u << 26))
        return fail(RL_E_INVALID, "scene too large: its records do not fit the 26 index bits of an object record");
    if (fs.n_clusters != 0 && fs.cluster_k != 10u && fs.cluster_k != 14u) {
#ifndef RL_CLUSTER_K
        return fail(RL_E_INVALID, "cluster size is not one the trace kernel's member rounds are unrolled for (RL_CLUSTER_K_CHOICES)");
#endif
    }
    // (on the device an object's group bits are the blob index of the record its hit is completed from, RlSceneView::records)
    for (size_t i = 0; i < fs.objects.size(); ++i) {
        const uint32_t bits = rl_f2u(fs.objects[i].w), kind = rl_object_surface(bits), group = rl_object_group(bits);
        const uint32_t index = kind == RL_SURFACE_SPHERE       ? group
                               : kind == RL_SURFACE_PARABOLOID ? lay.off_parabs + 3u * group
                               : kind == RL_SURFACE_HEX_PRISM  ? lay.off_prisms + (uint32_t)RL_PRISM_STRIDE * group
                                                               : lay.off_planes + 2u * group;
        blob[lay.off_objects + i].w = rl_u2f(rl_object_bits(kind, rl_object_material(bits), index));
    }
    lay.off_cie = (uint32_t)blob.size();
    const RlF4* cie = (const RlF4*)RL_CIE1931_XYZ0;
    blob.insert(blob.end(), cie, cie + RL_CIE_SAMPLES);
    lay.off_sphere_obj = (uint32_t)blob.size();
    const size_t so_f4 = (fs.sphere_obj.size() + 3) / 4;
    blob.resize(blob.size() + so_f4);
    std::memcpy(blob.data() + lay.off_sphere_obj, fs.sphere_obj.data(), fs.sphere_obj.size() * sizeof(uint32_t));
    lay.off_sphere_r2 = (uint32_t)blob.size();
    blob.resize(blob.size() + so_f4);
    for (size_t pos = 0; pos < fs.spheres.size(); ++pos) ((float*)(blob.data() + lay.off_sphere_r2))[pos] = fs.spheres[pos].w;
    lay.total_f4 = (uint32_t)blob.size();
    lay.n_direct = fs.n_direct;
    lay.n_direct_padded = fs.n_direct_padded;
    lay.cluster_base = fs.cluster_base;
    lay.n_clusters = fs.n_clusters;
    lay.cluster_k = fs.cluster_k;
    lay.n_cluster_groups = fs.n_cluster_groups;
    lay.n_prism_groups = fs.n_prism_groups;
    lay.n_cluster_supers = fs.n_cluster_supers;
    lay.super_g = fs.super_g;
    lay.n_planes = (uint32_t)(fs.planes.size() / 2);
    lay.n_parabs = (uint32_t)(fs.parabs.size() / 3);
    lay.n_prisms = (uint32_t)(fs.prisms.size() / RL_PRISM_STRIDE);
    lay.n_objects = (uint32_t)fs.objects.size();

    RlScene* s = new (std::nothrow) RlScene();
    if (!s) return fail(RL_E_INVALID, "out of host memory");
    s->device = device;
    s->lay = lay;
    s->staged_bytes = blob.size() * sizeof(RlF4);
    s->tables_bytes = (size_t)(lay.off_objects - lay.off_planes) * sizeof(RlF4);
    std::vector<RlF4> emitters;
    emitter_table(desc->objects, desc->n_objects, &emitters, &s->emitter_objects);
    std::vector<uint8_t> flags(desc->n_objects, (uint8_t)0);
    for (uint32_t object : s->emitter_objects) flags[object] = 1;
    s->ledger.alloc(&s->blob, s->staged_bytes, blob.data());
    if (!emitters.empty()) {
        s->ledger.alloc(&s->emitters, emitters.size() * sizeof(RlF4), emitters.data());
        s->ledger.alloc(&s->emitter_flags, flags.size(), flags.data());
    }
    return unit_created("scene upload", s, rl_scene_destroy, out);
}

namespace {
int sessions_quiesce(int device);
int render_end(RlTraceUnit* u);
}

int rl_scene_destroy(RlScene* scene) {
    if (!scene) return RL_OK;
    (void)hipSetDevice(scene->device);
    (void)sessions_quiesce(scene->device); // an open launch may still be reading the blob
    scene->ledger.release();
    delete scene;
    return RL_OK;
}

int rl_scene_intersect(const RlScene* scene, int primitive_fetch, const RlRay* rays, uint32_t n_rays, RlRayHit* hits) {
    const int rc = query_check(scene, primitive_fetch, rays, n_rays, hits);
    if (rc != RL_OK || n_rays == 0) return rc;
    return with_query_ctx(scene, [&](const CallCtx& c) -> int {
        return staged_chunks(c, n_rays, {staged_in(STAGING_RAYS, rays, sizeof(RlRay)), staged_out(STAGING_HITS, hits, sizeof(RlRayHit))},
                             [&](uint32_t, uint32_t k) -> int {
                                 return launch_persistent(c, g_query_kernels, scene, primitive_fetch, k, (const RlRay*)c.q->staging[STAGING_RAYS],
                                                          (RlRayHit*)c.q->staging[STAGING_HITS], k);
                             });
    });
}

int rl_scene_intersect_device(const RlScene* scene, int primitive_fetch, const RlRay* device_rays, uint32_t n_rays, RlRayHit* device_hits) {
    const int rc = query_check(scene, primitive_fetch, device_rays, n_rays, device_hits);
    if (rc != RL_OK || n_rays == 0) return rc;
    return with_query_ctx(scene, {"rl_scene_intersect_device", "rl_scene_intersect", {device_rays, device_hits}}, [&](const CallCtx& c) -> int {
        return launch_persistent(c, g_query_kernels, scene, primitive_fetch, n_rays, device_rays, device_hits, n_rays);
    });
}

// One byte per ray: the host form stages them through the hit records' buffer.
int rl_scene_occluded(const RlScene* scene, int primitive_fetch, const RlRay* rays, uint32_t n_rays, uint8_t* occluded) {
    const int rc = query_check(scene, primitive_fetch, rays, n_rays, occluded);
    if (rc != RL_OK || n_rays == 0) return rc;
    return with_query_ctx(scene, [&](const CallCtx& c) -> int {
        return staged_chunks(c, n_rays, {staged_in(STAGING_RAYS, rays, sizeof(RlRay)), staged_out(STAGING_HITS, occluded, sizeof(uint8_t))},
                             [&](uint32_t, uint32_t k) -> int {
                                 return launch_persistent(c, g_occlusion_kernels, scene, primitive_fetch, k, (const RlRay*)c.q->staging[STAGING_RAYS],
                                                          (uint8_t*)c.q->staging[STAGING_HITS], k);
                             });
    });
}

int rl_scene_occluded_device(const RlScene* scene, int primitive_fetch, const RlRay* device_rays, uint32_t n_rays, uint8_t* device_occluded) {
    const int rc = query_check(scene, primitive_fetch, device_rays, n_rays, device_occluded);
    if (rc != RL_OK || n_rays == 0) return rc;
    return with_query_ctx(scene, {"rl_scene_occluded_device", "rl_scene_occluded", {device_rays, device_occluded}}, [&](const CallCtx& c) -> int {
        return launch_persistent(c, g_occlusion_kernels, scene, primitive_fetch, n_rays, device_rays, device_occluded, n_rays);
    });
}

int rl_scene_camera_rays(const RlScene* scene, uint32_t width, uint32_t height, uint64_t seed, uint32_t stream, uint64_t first_path_index,
                         uint32_t n, RlCameraSample* samples) {
    const int rc = camera_check(scene, width, height, first_path_index, n, samples);
    if (rc != RL_OK || n == 0) return rc;
    return with_query_ctx(scene, [&](const CallCtx& c) -> int {
        return staged_chunks(c, n, {staged_out(STAGING_HITS, samples, sizeof(RlCameraSample))}, [&](uint32_t first, uint32_t k) -> int {
            return launch_camera(c, scene, width, height, seed, stream, first_path_index + first, (RlCameraSample*)c.q->staging[STAGING_HITS], k);
        });
    });
}

int rl_scene_camera_rays_device(const RlScene* scene, uint32_t width, uint32_t height, uint64_t seed, uint32_t stream,
                                uint64_t first_path_index, uint32_t n, RlCameraSample* device_samples) {
    const int rc = camera_check(scene, width, height, first_path_index, n, device_samples);
    if (rc != RL_OK || n == 0) return rc;
    return with_query_ctx(scene, {"rl_scene_camera_rays_device", "rl_scene_camera_rays", {device_samples}}, [&](const CallCtx& c) -> int {
        return launch_camera(c, scene, width, height, seed, stream, first_path_index, device_samples, n);
    });
}

int rl_scene_render_rays(const RlScene* scene, int primitive_fetch, uint64_t seed, uint32_t stream, uint64_t first_path_index,
                         uint32_t max_segments, const RlSpectralRay* rays, uint32_t n_rays, RlPathResult* results) {
    PathJob job{seed, stream, 0u};
    const int rc = paths_check(scene, primitive_fetch, rays, n_rays, results, first_path_index, max_segments, &job);
    if (rc != RL_OK || n_rays == 0) return rc;
    return with_query_ctx(scene, [&](const CallCtx& c) -> int {
        return staged_chunks(c, n_rays, {staged_in(STAGING_RAYS, rays, sizeof(RlSpectralRay)), staged_out(STAGING_HITS, results, sizeof(RlPathResult))},
                             [&](uint32_t first, uint32_t k) -> int {
                                 return launch_paths(c, scene, primitive_fetch, job, first_path_index + first, (const RlSpectralRay*)c.q->staging[STAGING_RAYS],
                                                     (RlPathResult*)c.q->staging[STAGING_HITS], k);
                             });
    });
}

int rl_scene_render_rays_device(const RlScene* scene, int primitive_fetch, uint64_t seed, uint32_t stream, uint64_t first_path_index,
                                uint32_t max_segments, const RlSpectralRay* device_rays, uint32_t n_rays, RlPathResult* device_results) {
    PathJob job{seed, stream, 0u};
    const int rc = paths_check(scene, primitive_fetch, device_rays, n_rays, device_results, first_path_index, max_segments, &job);
    if (rc != RL_OK || n_rays == 0) return rc;
    return with_query_ctx(scene, {"rl_scene_render_rays_device", "rl_scene_render_rays", {device_rays, device_results}}, [&](const CallCtx& c) -> int {
        return launch_paths(c, scene, primitive_fetch, job, first_path_index, device_rays, device_results, n_rays);
    });
}

int rl_scene_begin_paths(const RlScene* scene, uint64_t first_path_index, const RlSpectralRay* rays, uint32_t n, RlPathState* states) {
    const int rc = begin_check(scene, first_path_index, rays, n, states);
    if (rc != RL_OK || n == 0) return rc;
    return with_query_ctx(scene, [&](const CallCtx& c) -> int {
        return staged_chunks(c, n, {staged_in(STAGING_RAYS, rays, sizeof(RlSpectralRay)), staged_out(STAGING_STATES, states, sizeof(RlPathState))},
                             [&](uint32_t first, uint32_t k) -> int {
                                 return launch_begin(c, first_path_index + first, (const RlSpectralRay*)c.q->staging[STAGING_RAYS],
                                                     (RlPathState*)c.q->staging[STAGING_STATES], k);
                             });
    });
}

int rl_scene_begin_paths_device(const RlScene* scene, uint64_t first_path_index, const RlSpectralRay* device_rays, uint32_t n,
                                RlPathState* device_states) {
    int rc = begin_check(scene, first_path_index, device_rays, n, device_states);
    if (rc != RL_OK || n == 0) return rc;
    if ((rc = states_aligned(device_states, "rl_scene_begin_paths_device")) != RL_OK) return rc;
    return with_query_ctx(scene, {"rl_scene_begin_paths_device", "rl_scene_begin_paths", {device_rays, device_states}}, [&](const CallCtx& c) -> int {
        return launch_begin(c, first_path_index, device_rays, device_states, n);
    });
}

int rl_scene_step_paths(const RlScene* scene, int primitive_fetch, uint64_t seed, uint32_t stream, uint32_t flags, RlPathState* states,
                        uint32_t n, RlRayHit* hits) {
    const int rc = step_check(scene, primitive_fetch, flags, states, n);
    if (rc != RL_OK || n == 0) return rc;
    return with_query_ctx(scene, [&](const CallCtx& c) -> int {
        // (the caller's hits go in too: the slots of the states that are not stepped come back as they were)
        return staged_chunks(c, n, {staged_inout(STAGING_STATES, states, sizeof(RlPathState)), staged_inout(STAGING_HITS, hits, sizeof(RlRayHit))},
                             [&](uint32_t, uint32_t k) -> int {
                                 return launch_step(c, scene, primitive_fetch, seed, stream, flags, (RlPathState*)c.q->staging[STAGING_STATES],
                                                    hits ? (RlRayHit*)c.q->staging[STAGING_HITS] : nullptr, k);
                             });
    });
}

int rl_scene_step_paths_device(const RlScene* scene, int primitive_fetch, uint64_t seed, uint32_t stream, uint32_t flags,
                               RlPathState* device_states, uint32_t n, RlRayHit* device_hits) {
    int rc = step_check(scene, primitive_fetch, flags, device_states, n);
    if (rc != RL_OK || n == 0) return rc;
    if ((rc = states_aligned(device_states, "rl_scene_step_paths_device")) != RL_OK) return rc;
    return with_query_ctx(scene, {"rl_scene_step_paths_device", "rl_scene_step_paths", {device_states, device_hits}}, [&](const CallCtx& c) -> int {
        return launch_step(c, scene, primitive_fetch, seed, stream, flags, device_states, device_hits, n);
    });
}

int rl_scene_step_path_list_device(const RlScene* scene, int primitive_fetch, uint64_t seed, uint32_t stream, uint32_t flags,
                                   RlPathState* device_states, uint32_t n_states, const uint32_t* device_list, uint32_t n_list,
                                   RlRayHit* device_hits, uint32_t* device_live_list, uint32_t* n_live) {
    int rc = path_list_check(scene, primitive_fetch, flags, device_states, n_states, device_list, n_list);
    if (rc != RL_OK) return rc;
    if (n_live) *n_live = 0u;
    if (n_list == 0) return RL_OK;
    const char* what = "rl_scene_step_path_list_device";
    if ((rc = states_aligned(device_states, what)) != RL_OK) return rc;
    if ((rc = aligned_check(what, "a list", 4, {device_list, device_live_list})) != RL_OK) return rc;
    uint32_t total = 0; // (written by the call's copy, read behind with_query_ctx's synchronise)
    rc = with_query_ctx(scene, {what, "rl_scene_step_path_list", {device_states, device_hits, device_list, device_live_list}}, [&](const CallCtx& c) -> int {
        return launch_list_step(c, scene, primitive_fetch, seed, stream, flags, device_states, n_states, device_list, n_list, device_hits,
                                device_live_list, n_live ? &total : nullptr);
    });
    if (rc == RL_OK && n_live) *n_live = total;
    return rc;
}

// Not chunked (WholeArrays).
int rl_scene_step_path_list(const RlScene* scene, int primitive_fetch, uint64_t seed, uint32_t stream, uint32_t flags, RlPathState* states,
                            uint32_t n_states, const uint32_t* list, uint32_t n_list, RlRayHit* hits, uint32_t* live_list, uint32_t* n_live) {
    int rc = path_list_check(scene, primitive_fetch, flags, states, n_states, list, n_list);
    if (rc != RL_OK) return rc;
    if (n_live) *n_live = 0u;
    if (n_list == 0) return RL_OK;
    if ((rc = use_device(scene->device)) != RL_OK) return rc;
    // (the caller's hits go in too: the slots of the states that are not stepped come back as they were)
    Whole d_states = whole_inout(states, (size_t)n_states * sizeof(RlPathState)), d_hits = whole_inout(hits, (size_t)n_states * sizeof(RlRayHit));
    Whole d_list = whole_in(list, (size_t)n_list * sizeof(uint32_t)), d_live = whole_scratch(live_list, (size_t)n_list * sizeof(uint32_t));
    WholeArrays dev(&d_states, &d_hits, &d_list, &d_live);
    if ((rc = dev.allocate()) != RL_OK) return rc;
    uint32_t total = 0;
    rc = with_query_ctx(scene, [&](const CallCtx& c) -> int {
        const int r = dev.run(c.stream, [&]() -> int {
            return launch_list_step(c, scene, primitive_fetch, seed, stream, flags, (RlPathState*)d_states.dev, n_states, (const uint32_t*)d_list.dev,
                                    n_list, (RlRayHit*)d_hits.dev, (uint32_t*)d_live.dev, live_list || n_live ? &total : nullptr);
        });
        if (r != RL_OK) return r;
        RL_HIP(hipStreamSynchronize(c.stream)); // (`total` is known from here)
        if (live_list && total) RL_HIP(hipMemcpyAsync(live_list, d_live.dev, (size_t)total * sizeof(uint32_t), hipMemcpyDeviceToHost, c.stream));
        return RL_OK;
    });
    if (rc == RL_OK && n_live) *n_live = total;
    return rc;
}

int rl_scene_emitters(const RlScene* scene, uint32_t* objects, uint32_t cap, uint32_t* n_emitters) {
    if (!scene) return fail(RL_E_INVALID, "null scene");
    if (!n_emitters) return fail(RL_E_INVALID, "null output");
    const uint32_t n = (uint32_t)scene->emitter_objects.size();
    *n_emitters = n;
    if (n == 0) return RL_OK;
    if (!objects || cap < n) return fail(RL_E_INVALID, "index array too small for the scene's emitters");
    std::memcpy(objects, scene->emitter_objects.data(), n * sizeof(uint32_t));
    return RL_OK;
}

int rl_scene_light_paths_device(const RlScene* scene, int primitive_fetch, uint64_t seed, uint32_t stream, const RlPathState* device_states,
                                uint32_t n_states, const uint32_t* device_list, uint32_t n_list, const RlRayHit* device_hits,
                                RlLightSample* device_samples) {
    int rc = light_check(scene, primitive_fetch, device_states, n_states, device_list, n_list, device_hits, device_samples);
    if (rc != RL_OK || n_list == 0) return rc;
    const char* what = "rl_scene_light_paths_device";
    if ((rc = states_aligned(device_states, what)) != RL_OK) return rc;
    if ((rc = aligned_check(what, "the sample buffer", 16, {device_samples})) != RL_OK) return rc;
    if ((rc = aligned_check(what, "the list", 4, {device_list})) != RL_OK) return rc;
    return with_query_ctx(scene, {what, "rl_scene_light_paths", {device_states, device_hits, device_list, device_samples}}, [&](const CallCtx& c) -> int {
        return launch_light(c, scene, primitive_fetch, seed, stream, device_states, n_states, device_list, n_list, device_hits, device_samples);
    });
}

// Not chunked (WholeArrays).  The caller's samples go in too: the records of the states that are not listed come back as they were.
int rl_scene_light_paths(const RlScene* scene, int primitive_fetch, uint64_t seed, uint32_t stream, const RlPathState* states, uint32_t n_states,
                         const uint32_t* list, uint32_t n_list, const RlRayHit* hits, RlLightSample* samples) {
    int rc = light_check(scene, primitive_fetch, states, n_states, list, n_list, hits, samples);
    if (rc != RL_OK || n_list == 0) return rc;
    if (n_states == 0) return RL_OK; // (a given list of a state buffer without states: every entry is skipped)
    if ((rc = use_device(scene->device)) != RL_OK) return rc;
    Whole d_states = whole_in(states, (size_t)n_states * sizeof(RlPathState)), d_hits = whole_in(hits, (size_t)n_states * sizeof(RlRayHit));
    Whole d_samples = whole_inout(samples, (size_t)n_states * sizeof(RlLightSample)), d_list = whole_in(list, (size_t)n_list * sizeof(uint32_t));
    WholeArrays dev(&d_states, &d_hits, &d_samples, &d_list);
    if ((rc = dev.allocate()) != RL_OK) return rc;
    return with_query_ctx(scene, [&](const CallCtx& c) -> int {
        return dev.run(c.stream, [&]() -> int {
            return launch_light(c, scene, primitive_fetch, seed, stream, (const RlPathState*)d_states.dev, n_states, (const uint32_t*)d_list.dev, n_list,
                                (const RlRayHit*)d_hits.dev, (RlLightSample*)d_samples.dev);
        });
    });
}

// ---- TraceUnit ----------------------------------------------------------------------------------

int rl_trace_unit_create(int device, uint32_t id, uint32_t width, uint32_t height, uint32_t n_photons,
                         RlTraceUnit** out) {
    RlTraceUnit* u = nullptr; // (value-initialised: no launch yet, nothing tuned, no time)
    int rc = unit_new("trace unit", device, width, height, n_photons, out, &u);
    if (rc != RL_OK) return rc;
    u->id = id;
    u->n_photons = n_photons;
    u->fetch = RL_FETCH_LDS;
    u->cu_count = 256;
    u->ledger.alloc_zeroed(&u->photons, (size_t)n_photons * sizeof(RlMappedPhoton)); // MappedPhoton::new
    u->ledger.alloc_zeroed(&u->queue, 3 * sizeof(unsigned long long));
    u->ledger.stream(&u->stream);
    u->ledger.event(&u->rendered);
    if ((rc = unit_created("trace unit allocation", u, rl_trace_unit_destroy, out)) != RL_OK) return rc;
    if ((rc = cu_count_of(device, &u->cu_count)) != RL_OK) {
        *out = nullptr;
        rl_trace_unit_destroy(u);
    }
    return rc;
}

int rl_trace_unit_destroy(RlTraceUnit* u) {
    if (!u) return RL_OK;
    (void)hipSetDevice(u->device);
    (void)render_end(u); // a render that was begun writes to this unit's photons until it is complete
    u->ledger.release();
    delete u;
    return RL_OK;
}

int rl_trace_unit_set_fetch(RlTraceUnit* u, int primitive_fetch) {
    if (!u) return fail(RL_E_INVALID, "null trace unit");
    if (primitive_fetch != RL_FETCH_LDS && primitive_fetch != RL_FETCH_GLOBAL) return fail(RL_E_INVALID, "unknown fetch mode");
    u->fetch = primitive_fetch;
    return RL_OK;
}

// ---- wavelength importance sampling (rl_wavelength.h) ---------------------------------------------

int rl_wavelength_importance_cie1931(double* out) {
    if (!out) return fail(RL_E_INVALID, "null output");
    rl_wavelength_cie_importance(out);
    return RL_OK;
}

// The checks of rl_wavelength_table_create behind its null-output check, in the header's order, and the table itself (513 floats).
// Host arithmetic only.  Internal (not in the C header): rl_app.cpp checks an RlWavelengthSampling with it before any device work.
extern "C" int rl_internal_wavelength_rule(const double* importance, uint32_t n_nodes, double uniform_share, float* table) {
    if (n_nodes < 2u || n_nodes > RL_WAVELENGTH_MAX_NODES) return fail(RL_E_INVALID, "wavelength table: n_nodes must be 2 .. 4096");
    if (!(uniform_share > 0.0 && uniform_share <= 1.0)) return fail(RL_E_INVALID, "wavelength table: uniform_share must be in (0, 1]");
    switch (rl_wavelength_table_rule(importance, n_nodes, uniform_share, table)) {
    case RL_WAVELENGTH_OK: return RL_OK;
    case RL_WAVELENGTH_OVERFLOW: return fail(RL_E_INVALID, "wavelength table: the sum of the importance overflows");
    default: return fail(RL_E_INVALID, "wavelength table: the quantiles do not increase in f32 (uniform_share is too small for this importance)");
    }
}

int rl_wavelength_table_create(int device, const double* importance, uint32_t n_nodes, double uniform_share, RlWavelengthTable** out) {
    if (!out) return fail(RL_E_INVALID, "null output handle");
    *out = nullptr;
    RlWavelengthTable* t = new (std::nothrow) RlWavelengthTable();
    if (!t) return fail(RL_E_INVALID, "out of host memory");
    int rc = rl_internal_wavelength_rule(importance, n_nodes, uniform_share, t->host);
    if (rc == RL_OK) rc = use_device(device);
    if (rc != RL_OK) {
        delete t;
        return rc;
    }
    static std::atomic<uint64_t> next_id{1};
    t->device = device;
    t->id = next_id.fetch_add(1, std::memory_order_relaxed);
    t->ledger.alloc(&t->table, sizeof t->host, t->host);
    return unit_created("wavelength table allocation", t, rl_wavelength_table_destroy, out);
}

int rl_wavelength_table_destroy(RlWavelengthTable* t) {
    if (!t) return RL_OK;
    (void)hipSetDevice(t->device);
    t->ledger.release();
    delete t;
    return RL_OK;
}

int rl_wavelength_table_download(RlWavelengthTable* t, float* quantiles, float* weights) {
    if (!t) return fail(RL_E_INVALID, "null wavelength table");
    const int rc = use_device(t->device);
    if (rc != RL_OK) return rc;
    return download(nullptr, {{t->table, quantiles, (RL_WAVELENGTH_BINS + 1) * sizeof(float)},
                              {t->table + (RL_WAVELENGTH_BINS + 1), weights, RL_WAVELENGTH_BINS * sizeof(float)}});
}

int rl_trace_unit_set_wavelengths(RlTraceUnit* u, const RlWavelengthTable* table) {
    if (!u) return fail(RL_E_INVALID, "null trace unit");
    if (table && table->device != u->device) return fail(RL_E_STATE, "wavelength table and trace unit live on different devices");
    if (u->ticket.pending) return fail(RL_E_STATE, "the trace unit has a render that was begun and not ended");
    u->wavelengths = table;
    return RL_OK;
}

int rl_trace_unit_render_async(RlTraceUnit* u, const RlScene* scene, uint64_t seed, uint32_t stream, uint64_t first_path_index) {
    if (!u || !scene) return fail(RL_E_INVALID, "null handle");
    int rc = use_device(u->device);
    if (rc != RL_OK) return rc;
    return launch_trace(u, scene, u->photons, nullptr, seed, stream, first_path_index, u->n_photons);
}

namespace {

// ---- sessions: open launches (rl_kernels.hip.h, RlOpenDev / RlOpenCtl) ---------------------------------------------
// Blocking render calls of at most RL_SESSION_MAX_PATHS paths are APPENDED to a trace kernel that is already running
// on the device whenever there is one that still accepts work (same scene, seed, stream, image size, fetch mode,
// fused or not); otherwise the call starts such a kernel with itself as the first job.  Each call returns as soon as
// ITS paths are finished -- the kernel goes on with the other callers' -- so the drain tail of one 524,288-path batch
// overlaps the next batches instead of idling the chip, and nothing is launched per call.  A kernel stays open while
// calls are still finishing their last paths (their callers come back with more) and for a grace period after the
// last one, then closes itself; a call that arrives too late for it starts the next one, whose workgroups move onto
// the CUs as the closed one's drain.  The calls also exist in two halves (begin / end, `Ticket`): whoever uses a
// begun render's result next ends it.

struct Session {
    hipStream_t stream = nullptr;
    RlOpenDev* od = nullptr;
    RlOpenCtl* ctl = nullptr;     // pinned, coherent host memory
    RlOpenCtl* ctl_dev = nullptr; // the same memory as the device addresses it
    unsigned long long* counters = nullptr; // [unused, segments, paths] of the running kernel
    hipEvent_t start = nullptr, stop = nullptr;
    bool launched = false; // a kernel was launched and its counters are not harvested yet
    bool open = false;     // the host may still try to append
    uint32_t n = 0;        // jobs appended so far
    int waiters = 0;       // calls that have not yet read their completion flag (ctl must not be recycled under them)
    const void* tuned_kernel = nullptr; // launch configuration last set up for this slot
    size_t tuned_dyn = 0;
    int tuned_per_cu = 1;
    const RlScene* scene = nullptr;
    uint64_t seed = 0;
    uint32_t stream_id = 0, width = 0, height = 0;
    int fetch = 0;
    bool fused = false;
    uint64_t wavelengths = 0; // the id of the units' wavelength table (0: none): calls with another one do not join
    // who the running kernel works for: (a unit's counters, paths of its call) per job; its run time is split by paths
    std::vector<std::pair<std::shared_ptr<UnitCounters>, uint64_t>> shares;
};

struct DeviceSessions {
    std::mutex lock;
    std::condition_variable changed;
    Session s[4];
    bool ready = false;
    uint64_t launches = 0;
    uint64_t histogram[RL_OPEN_CAP + 1] = {}; // finished kernels by number of calls they carried
    double presync_us = 0.0, admit_us = 0.0, wait_us = 0.0; // where the calls spent their time (RL_OPEN_LAUNCH_TIMING=1 prints it)
    uint64_t calls = 0, starts = 0;
};

DeviceSessions* sessions_of(int device) {
    static DeviceSessions all[64];
    return &all[device >= 0 && device < 64 ? device : 0];
}

inline uint32_t host_load(const uint32_t* p) { return __atomic_load_n(p, __ATOMIC_SEQ_CST); }

int sessions_setup(DeviceSessions* d) { // under d->lock, device current
    if (d->ready) return RL_OK;
    int least = 0, greatest = 0;
    RL_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
    for (Session& x : d->s) {
        // a priority of its own = a hardware queue of its own: the streams of the plot / gather / tonemap kernels must
        // never queue up behind a resident trace kernel (they run beside it in the registers it leaves free)
        if (hipStreamCreateWithPriority(&x.stream, hipStreamNonBlocking, least) != hipSuccess) { // (no priorities here: a plain stream)
            (void)hipGetLastError();
            RL_HIP(hipStreamCreateWithFlags(&x.stream, hipStreamNonBlocking));
        }
        RL_HIP(hipMalloc((void**)&x.od, sizeof(RlOpenDev)));
        RL_HIP(hipHostMalloc((void**)&x.ctl, sizeof(RlOpenCtl), hipHostMallocCoherent | hipHostMallocMapped));
        RL_HIP(hipHostGetDevicePointer((void**)&x.ctl_dev, x.ctl, 0));
        RL_HIP(hipMalloc((void**)&x.counters, 3 * sizeof(unsigned long long)));
        RL_HIP(hipEventCreate(&x.start));
        RL_HIP(hipEventCreate(&x.stop));
    }
    d->ready = true;
    return RL_OK;
}

// The kernel of session x has ended (or was never launched): add its counters to the device's tally.
int session_harvest(DeviceSessions* d, Session& x) {
    if (!x.launched) return RL_OK;
    RL_HIP(hipStreamSynchronize(x.stream));
    float ms = 0.0f;
    RL_HIP(hipEventElapsedTime(&ms, x.start, x.stop));
    uint64_t total = 0;
    for (const auto& sh : x.shares) total += sh.second;
    for (const auto& sh : x.shares) // every unit gets the part of the kernel's time that its paths are of the kernel's paths
        if (total) sh.first->kernel_ns += (uint64_t)((double)ms * 1.0e6 * ((double)sh.second / (double)total));
    x.shares.clear();
    d->launches += 1;
    const uint32_t carried = host_load(&x.ctl->final_at);
    d->histogram[carried <= RL_OPEN_CAP ? carried : 0] += 1;
    x.launched = false;
    x.open = false;
    return RL_OK;
}

// Waits until no session kernel runs on `device` and credits their run time to the units they worked for.  The waiting
// happens OUTSIDE the device's lock: other threads' render calls go on being admitted meanwhile -- to the
// kernels that are running, or to new ones, which this call then does not wait for.
int sessions_quiesce(int device) {
    DeviceSessions* d = sessions_of(device);
    hipStream_t streams[4];
    int n = 0;
    {
        std::lock_guard<std::mutex> guard(d->lock);
        if (!d->ready) return RL_OK;
        for (Session& x : d->s)
            if (x.launched) streams[n++] = x.stream;
    }
    for (int i = 0; i < n; ++i) RL_HIP(hipStreamSynchronize(streams[i]));
    std::lock_guard<std::mutex> guard(d->lock);
    for (Session& x : d->s) {
        if (!x.launched || hipStreamQuery(x.stream) != hipSuccess) continue; // restarted meanwhile: its next harvest counts it
        const int rc = session_harvest(d, x);
        if (rc != RL_OK) return rc;
    }
    return RL_OK;
}

int session_start(DeviceSessions* d, Session& x, RlTraceUnit* u, const RlScene* scene, bool fused, uint64_t seed, uint32_t stream_id,
                  const RlJobEntry& first) {
    int rc = session_harvest(d, x);
    if (rc != RL_OK) return rc;
    x.scene = scene;
    x.seed = seed;
    x.stream_id = stream_id;
    x.width = u->width;
    x.height = u->height;
    x.fetch = u->fetch;
    x.fused = fused;
    x.wavelengths = u->wavelengths ? u->wavelengths->id : 0u;
    RlTraceJob job;
    job.width = u->width;
    job.height = u->height;
    job.aspect_ratio = (float)u->width / (float)u->height;
    job.stream = stream_id;
    job.seed = seed;
    job.first_path = 0;
    job.n_paths = 0;
    static const uint32_t grace_us = getenv("RL_OPEN_LAUNCH_GRACE_US") ? (uint32_t)atoi(getenv("RL_OPEN_LAUNCH_GRACE_US")) : 150u;
    job.grace_ticks = grace_us * 100u; // ticks of wall_clock64() (100 MHz) an idle open launch waits for another call
    job.reserved = 0;
    job.wm1 = (float)(int)u->width - 1.0f;
    job.hm1 = (float)(int)u->height - 1.0f;
    const size_t scratch_bytes = (RL_TRACE_BLOCK / 64) * sizeof(RlWaveScratch) + sizeof(RlOpenWg) + ring_t_bytes(scene);
    size_t blob_bytes = 0;
    const int stage = stage_of(scene, u->fetch, scratch_bytes, &blob_bytes);
    const float* wl = u->wavelengths ? u->wavelengths->table : nullptr;
    const TraceKernel plain = wl ? nullptr : trace_kernel_variant(stage, fused, true, scene->lay.prism_cylinders != 0u);
    const TraceKernelWl sampled = wl ? trace_kernel_variant_wl(stage, fused, true, scene->lay.prism_cylinders != 0u) : nullptr;
    const void* kernel = wl ? (const void*)sampled : (const void*)plain;
    const size_t dyn = scratch_bytes + blob_bytes;
    if (x.tuned_kernel != kernel || x.tuned_dyn != dyn) { // once per (slot, variant, scene size)
        RL_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        int n = 1;
        RL_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, RL_TRACE_BLOCK, dyn));
        x.tuned_per_cu = n < 1 ? 1 : n;
        x.tuned_kernel = kernel;
        x.tuned_dyn = dyn;
    }
    const int per_cu = x.tuned_per_cu;
    std::memset(x.ctl, 0, sizeof(RlOpenCtl));
    x.ctl->jobs[0] = first;
    x.ctl->closed_at = RL_OPEN_NONE;
    x.ctl->final_at = RL_OPEN_NONE;
    __atomic_store_n(&x.ctl->published, 1u, __ATOMIC_SEQ_CST);
    x.n = 1;
    RL_HIP(hipMemsetAsync(x.od, 0, sizeof(RlOpenDev), x.stream));
    RL_HIP(hipMemsetAsync(x.counters, 0, 3 * sizeof(unsigned long long), x.stream));
    RL_HIP(hipEventRecord(x.start, x.stream));
    if (wl)
        hipLaunchKernelGGL(sampled, dim3((unsigned)(u->cu_count * per_cu)), dim3(RL_TRACE_BLOCK), dyn, x.stream, scene->blob, scene->lay, job,
                           (RlMappedPhoton*)nullptr, (float*)nullptr, x.counters, (const RlJobEntry*)x.od->jobs, x.od, x.ctl_dev, wl);
    else
        hipLaunchKernelGGL(plain, dim3((unsigned)(u->cu_count * per_cu)), dim3(RL_TRACE_BLOCK), dyn, x.stream, scene->blob, scene->lay, job,
                           (RlMappedPhoton*)nullptr, (float*)nullptr, x.counters, (const RlJobEntry*)x.od->jobs, x.od, x.ctl_dev);
    RL_HIP(hipGetLastError());
    RL_HIP(hipEventRecord(x.stop, x.stream));
    x.launched = true;
    x.open = true;
    return RL_OK;
}

// Appends `e` to the running kernel of x.  Returns the job index, or -1 when the kernel had already closed.
int session_append(Session& x, const RlJobEntry& e) {
    const uint32_t k = x.n;
    x.ctl->jobs[k] = e;
    __atomic_store_n(&x.ctl->done[k], 0u, __ATOMIC_RELAXED);
    __atomic_store_n(&x.ctl->published, k + 1u, __ATOMIC_SEQ_CST);
    __atomic_thread_fence(__ATOMIC_SEQ_CST);
    for (uint64_t spins = 0;; ++spins) {
        const uint32_t closed_at = host_load(&x.ctl->closed_at);
        if (closed_at == RL_OPEN_NONE || closed_at > k) break; // it had not closed when the entry became visible, or re-opened
        const uint32_t final_at = host_load(&x.ctl->final_at);
        if (final_at != RL_OPEN_NONE && final_at <= k) return -1;
        if (spins > 1000000 && hipStreamQuery(x.stream) != hipErrorNotReady) return -1; // the kernel is gone (an error surfaces later)
        __builtin_ia32_pause();
    }
    x.n = k + 1u;
    return (int)k;
}

// Blocks until job k of session x is complete.
int session_wait(Session& x, uint32_t k) {
    auto last_query = std::chrono::steady_clock::now();
    for (uint64_t spins = 0;; ++spins) {
        if (host_load(&x.ctl->done[k]) != 0u) return RL_OK;
        if (spins < 4000) {
            __builtin_ia32_pause();
        } else if ((spins & 255u) == 0u && std::chrono::steady_clock::now() - last_query > std::chrono::milliseconds(20)) {
            // rarely (the query is not cheap while a kernel runs): has the kernel died or ended under the call?
            last_query = std::chrono::steady_clock::now();
            const hipError_t q = hipStreamQuery(x.stream);
            if (q == hipSuccess) { // the kernel has ended: it reported every accepted job before that
                if (host_load(&x.ctl->done[k]) != 0u) return RL_OK;
                return fail(RL_E_STATE, "an open trace launch ended without completing one of its calls");
            }
            if (q != hipErrorNotReady) return fail(RL_E_HIP, std::string("open trace launch: ") + hipGetErrorString(q));
        } else if (spins < 4000 + 64) {
            std::this_thread::yield();
        } else {
            // Round 6: a call that is not done after ~50 us of spinning and yielding SLEEPS between looks.  Yielding for ever is fine
            // while there are at most as many waiting workers as cores; the reference starts num_cpus::get() workers (app.rs:55), a
            // host may have fewer cores than that per GPU, and waiting threads that keep yielding then take the cores from the ones
            // that have tasks to issue (un-fused, workers that wait for their own batch: 14.1 Grays/s at 16 workers, 5.3 at 64 on 16 cores).
            static thread_local bool slack_set = false;
            if (!slack_set) {
                prctl(PR_SET_TIMERSLACK, 2000UL, 0UL, 0UL, 0UL); // (the default slack of 50 us would triple a 25 us sleep)
                slack_set = true;
            }
            std::this_thread::sleep_for(std::chrono::microseconds(25));
        }
    }
}

// First half of a blocking render served by an open launch: appends the call (or starts a launch with it) and leaves a
// ticket in the unit.
int session_begin(RlTraceUnit* u, const RlScene* scene, RlPlotUnit* plot, uint64_t seed, uint32_t stream_id, uint64_t first_path_index,
                  uint64_t n_paths) {
    // What the call's target is still being read or cleared by (a plot of the unit's previous photons, the gather's
    // clear of the plot buffer) must be over before a kernel that is already running may write to it.
    const auto t0 = std::chrono::steady_clock::now();
    if (plot) {
        RL_HIP(hipEventSynchronize(plot->cleared));
        // ... and whatever else still reads or writes the buffer on the plot unit's own stream (rl_plot_unit_add, the RCCL
        // reduce, an upload): a splat of the running kernel must not race them
        RL_HIP(hipStreamSynchronize(plot->stream));
    } else {
        RL_HIP(hipStreamSynchronize(u->stream));
    }
    const auto t1 = std::chrono::steady_clock::now();
    RlJobEntry e;
    e.target = plot ? (void*)plot->xyz : (void*)u->photons;
    e.first_path = first_path_index;
    e.start = 0;
    e.end = n_paths;
    DeviceSessions* d = sessions_of(u->device);
    Session* mine = nullptr;
    int k = -1;
    {
        std::unique_lock<std::mutex> guard(d->lock);
        int rc = sessions_setup(d);
        if (rc != RL_OK) return rc;
        for (;;) {
            for (Session& x : d->s) // a running kernel that takes this call?
                if (x.open && x.n < RL_OPEN_CAP && x.scene == scene && x.seed == seed && x.stream_id == stream_id && x.width == u->width &&
                    x.height == u->height && x.fetch == u->fetch && x.fused == (plot != nullptr) && x.wavelengths == (u->wavelengths ? u->wavelengths->id : 0u)) {
                    k = session_append(x, e);
                    if (k >= 0) mine = &x, x.waiters += 1, x.shares.emplace_back(u->counters, n_paths);
                    else x.open = false;
                    break;
                }
            if (mine) break;
            for (Session& x : d->s) // a kernel closes itself; the host learns of it here (or when an append is turned down)
                if (x.open && host_load(&x.ctl->final_at) != RL_OPEN_NONE) x.open = false;
            for (Session& x : d->s) // no: start one in a slot whose kernel has ended
                if (!x.open && x.waiters == 0 && (!x.launched || hipStreamQuery(x.stream) == hipSuccess)) {
                    rc = session_start(d, x, u, scene, plot != nullptr, seed, stream_id, e);
                    if (rc != RL_OK) return rc;
                    mine = &x;
                    x.waiters += 1;
                    x.shares.emplace_back(u->counters, n_paths);
                    k = 0;
                    break;
                }
            if (mine) break;
            bool retry = false; // an open session that is full: close it to the host
            for (Session& x : d->s)
                if (x.open && x.n >= RL_OPEN_CAP) x.open = false, retry = true;
            if (retry) continue;
            // Every slot is taken by another (scene, seed, stream, size, fetch, fused, wavelength table) combination.  A slot nobody waits
            // on frees itself (its kernel closes after a grace period), but one that carries begun renders stays until
            // they are ended -- possibly by this very thread (a fifth combination begun without ending an
            // earlier one used to spin here for ever).  If all of them do, the call gets a launch of its own instead.
            bool all_pinned = true;
            for (Session& x : d->s)
                if (x.waiters == 0) all_pinned = false;
            if (all_pinned) return RL_SESSIONS_PINNED;
            d->changed.wait_for(guard, std::chrono::microseconds(50));
        }
    }
    Ticket& t = plot ? plot->ticket : u->ticket;
    t.pending = true;
    t.session = mine;
    t.job = (uint32_t)k;
    t.paths = n_paths;
    t.device = u->device;
    t.counters = u->counters;
    t.presync_us = std::chrono::duration<double, std::micro>(t1 - t0).count();
    t.admit_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t1).count();
    return RL_OK;
}

// Second half: waits until the call's paths are finished.
int session_end(Ticket& t) {
    Session* mine = t.session;
    const uint32_t k = t.job;
    DeviceSessions* d = sessions_of(t.device);
    const auto t2 = std::chrono::steady_clock::now();
    int rc = session_wait(*mine, k);
    const uint64_t job_segments = host_load(&mine->ctl->segs[k]);
    {
        const auto t3 = std::chrono::steady_clock::now();
        std::lock_guard<std::mutex> guard(d->lock);
        mine->waiters -= 1;
        d->changed.notify_all(); // a slot may have become free for a thread waiting in session_begin
        d->presync_us += t.presync_us;
        d->admit_us += t.admit_us;
        d->wait_us += std::chrono::duration<double, std::micro>(t3 - t2).count();
        d->calls += 1;
    }
    t.session = nullptr;
    t.pending = false;
    if (rc == RL_OK) {
        t.counters->paths += t.paths;
        t.counters->segments += job_segments;
    }
    t.counters.reset();
    return rc;
}

#define RL_SESSION_MAX_PATHS (1ull << 28) // per call: its segment count must fit 32 bits

// The two halves of the blocking render of both kinds: un-fused (plot == nullptr, n_paths = the unit's batch) and fused.
int render_begin(RlTraceUnit* u, const RlScene* scene, RlPlotUnit* plot, uint64_t seed, uint32_t stream, uint64_t first_path_index,
                 uint64_t n_paths) {
    int rc = use_device(u->device);
    if (rc != RL_OK) return rc;
    if (!plot && u->ticket.pending) return fail(RL_E_STATE, "the trace unit has a render that was begun and not ended");
    if (plot && (rc = plot_settle(plot)) != RL_OK) return rc; // the plot unit's previous begun render first
    if (n_paths == 0) return RL_OK;
    if (scene->device != u->device) return fail(RL_E_STATE, "scene and trace unit live on different devices");
    if (first_path_index + n_paths < first_path_index || first_path_index + n_paths == ~0ull)
        return fail(RL_E_INVALID, "path indices must stay below 2^64 - 1");
    if (n_paths % 64 == 0 && n_paths < RL_SESSION_MAX_PATHS) {
        rc = session_begin(u, scene, plot, seed, stream, first_path_index, n_paths);
        if (rc != RL_SESSIONS_PINNED) return rc;
    }
    // a ragged or a huge batch, or no open launch to be had (rl_trace_unit_render_begin in robigo_luculenta.h): a launch of
    // its own on the unit's stream (a fused one is waited for by the plot unit's stream)
    rc = launch_trace(u, scene, plot ? nullptr : u->photons, plot, seed, stream, first_path_index, n_paths);
    if (rc != RL_OK) return rc;
    Ticket& t = plot ? plot->ticket : u->ticket;
    t.pending = true;
    t.session = nullptr;
    t.device = u->device;
    return RL_OK;
}

// Ends the fused render that splats into `plot`, if one was begun: everything that reads, clears or adds to the buffer
// calls this first.
int plot_settle(RlPlotUnit* plot) {
    Ticket& t = plot->ticket;
    if (!t.pending) return RL_OK;
    int rc = use_device(plot->device);
    if (rc != RL_OK) return rc;
    if (t.session) return session_end(t);
    t.pending = false;
    RL_HIP(hipStreamSynchronize(plot->stream)); // it waits for the launch (launch_trace)
    return RL_OK;
}

// Ends the un-fused render begun on `u`, if any.
int render_end(RlTraceUnit* u) {
    int rc = use_device(u->device);
    if (rc != RL_OK) return rc;
    Ticket& t = u->ticket;
    if (!t.pending) return RL_OK;
    if (t.session) {
        if ((rc = session_end(t)) != RL_OK) return rc;
        RL_HIP(hipEventRecord(u->rendered, u->stream)); // PlotUnit::plot waits for this (complete already)
        return RL_OK;
    }
    t.pending = false;
    RL_HIP(hipStreamSynchronize(u->stream));
    return RL_OK;
}

} // namespace

// TraceUnit::render as the reference's workers call it: blocking, one 524,288-path batch per call (trace_unit.rs:67).
// That batch is 0.15 ms of MI355X work followed by ~0.2 ms in which the launch waits for its longest paths, so the
// calls that are in flight at the same time -- the reference runs one per worker thread -- share OPEN launches (above).
// Results are those of separate launches, bit for bit: a path is a pure function of (seed, stream, path index).
int rl_trace_unit_render(RlTraceUnit* u, const RlScene* scene, uint64_t seed, uint32_t stream, uint64_t first_path_index) {
    if (!u || !scene) return fail(RL_E_INVALID, "null handle");
    const int rc = render_begin(u, scene, nullptr, seed, stream, first_path_index, u->n_photons);
    return rc != RL_OK ? rc : render_end(u);
}

int rl_trace_unit_render_begin(RlTraceUnit* u, const RlScene* scene, uint64_t seed, uint32_t stream, uint64_t first_path_index) {
    if (!u || !scene) return fail(RL_E_INVALID, "null handle");
    return render_begin(u, scene, nullptr, seed, stream, first_path_index, u->n_photons);
}

int rl_trace_unit_render_end(RlTraceUnit* u) {
    if (!u) return fail(RL_E_INVALID, "null trace unit");
    return render_end(u);
}

namespace {
int check_fused(const RlTraceUnit* u, const RlScene* scene, const RlPlotUnit* plot) {
    if (!u || !scene || !plot) return fail(RL_E_INVALID, "null handle");
    return match_check(plot, u);
}
} // namespace

int rl_trace_unit_render_fused_sync(RlTraceUnit* u, const RlScene* scene, RlPlotUnit* plot, uint64_t seed, uint32_t stream,
                                    uint64_t first_path_index, uint64_t n_paths) {
    int rc = check_fused(u, scene, plot);
    if (rc == RL_OK) rc = render_begin(u, scene, plot, seed, stream, first_path_index, n_paths);
    return rc != RL_OK ? rc : plot_settle(plot);
}

int rl_trace_unit_render_fused_begin(RlTraceUnit* u, const RlScene* scene, RlPlotUnit* plot, uint64_t seed, uint32_t stream,
                                     uint64_t first_path_index, uint64_t n_paths) {
    const int rc = check_fused(u, scene, plot);
    return rc != RL_OK ? rc : render_begin(u, scene, plot, seed, stream, first_path_index, n_paths);
}

int rl_trace_unit_render_fused(RlTraceUnit* u, const RlScene* scene, RlPlotUnit* plot, uint64_t seed, uint32_t stream,
                               uint64_t first_path_index, uint64_t n_paths) {
    int rc = check_fused(u, scene, plot);
    if (rc == RL_OK) rc = use_device(u->device);
    if (rc != RL_OK) return rc;
    return launch_trace(u, scene, nullptr, plot, seed, stream, first_path_index, n_paths);
}

int rl_trace_unit_sync(RlTraceUnit* u) {
    if (!u) return fail(RL_E_INVALID, "null trace unit");
    int rc = render_end(u); // also ends a render that was begun
    if (rc != RL_OK) return rc;
    RL_HIP(hipStreamSynchronize(u->stream));
    return drain_events(u);
}

int rl_trace_unit_photons(RlTraceUnit* u, RlMappedPhoton* out) {
    if (!u || !out) return fail(RL_E_INVALID, "null argument");
    int rc = use_device(u->device);
    if (rc != RL_OK) return rc;
    if ((rc = render_end(u)) != RL_OK) return rc; // a render that was begun: its photons are complete after this
    return download(u->stream, {{u->photons, out, (size_t)u->n_photons * sizeof(RlMappedPhoton)}});
}

int rl_trace_unit_stats(RlTraceUnit* u, uint64_t* paths, uint64_t* segments, double* kernel_ms) {
    if (!u) return fail(RL_E_INVALID, "null trace unit");
    int rc = render_end(u); // renders that were begun are counted when they end
    if (rc != RL_OK) return rc;
    RL_HIP(hipStreamSynchronize(u->stream));
    if ((rc = drain_events(u)) != RL_OK) return rc;
    unsigned long long q[3];
    RL_HIP(hipMemcpy(q, u->queue, sizeof q, hipMemcpyDeviceToHost));
    // Calls served by open launches are counted per call (session_*); the run time of such a launch, which serves many
    // units at once, is split among them by paths when it has ended (session_harvest).
    if ((rc = sessions_quiesce(u->device)) != RL_OK) return rc;
    if (segments) *segments = q[1] + u->counters->segments.load();
    if (paths) *paths = q[2] + u->counters->paths.load();
    if (kernel_ms) *kernel_ms = u->kernel_ms + (double)u->counters->kernel_ns.load() * 1.0e-6;
    return RL_OK;
}

// ---- PlotUnit -----------------------------------------------------------------------------------

int rl_plot_unit_create(int device, uint32_t id, uint32_t width, uint32_t height, float* external_xyz, RlPlotUnit** out) {
    RlPlotUnit* u = nullptr;
    const int rc = unit_new("plot unit", device, width, height, 1u, out, &u);
    if (rc != RL_OK) return rc;
    u->id = id;
    u->xyz = external_xyz; // (the caller's: not entered in the ledger)
    if (!external_xyz) u->ledger.alloc_zeroed(&u->xyz, (size_t)width * height * 3 * sizeof(float));
    u->ledger.alloc(&u->cie, sizeof RL_CIE1931_XYZ0, RL_CIE1931_XYZ0);
    u->ledger.stream(&u->stream);
    u->ledger.event(&u->plotted);
    u->ledger.event(&u->ready);
    u->ledger.event(&u->cleared);
    u->ledger.event(&u->tail);
    return unit_created("plot unit allocation", u, rl_plot_unit_destroy, out);
}

int rl_plot_unit_destroy(RlPlotUnit* u) {
    if (!u) return RL_OK;
    (void)hipSetDevice(u->device);
    (void)plot_settle(u); // a fused render that was begun splats into this buffer until it is complete
    u->ledger.release();
    delete u;
    return RL_OK;
}

int rl_plot_unit_plot(RlPlotUnit* u, RlTraceUnit* const* trace_units, uint32_t n_trace_units) {
    if (!u || (!trace_units && n_trace_units)) return fail(RL_E_INVALID, "null argument");
    int cus = 256;
    int rc = enter_device(u->device, &cus);
    if (rc != RL_OK) return rc;
    if ((rc = plot_settle(u)) != RL_OK) return rc; // a fused render begun into this buffer ends first
    const float aspect = (float)u->width / (float)u->height; // plot_unit.rs:48
    for (uint32_t k = 0; k < n_trace_units; ++k) {           // app.rs:138-140
        RlTraceUnit* t = trace_units[k];
        if (!t || t->device != u->device) return fail(RL_E_STATE, "trace unit missing or on another device");
        if ((rc = render_end(t)) != RL_OK) return rc;          // a render that was begun: its photons are complete after this
        RL_HIP(hipStreamWaitEvent(u->stream, t->rendered, 0)); // mapped_photons complete (a no-op after a synchronous render)
        hipLaunchKernelGGL(rl_plot_kernel, dim3(grid_for(t->n_photons, cus)), dim3(RL_BLOCK), 0, u->stream, t->photons,
                           t->n_photons, u->cie, u->width, u->height, aspect, u->xyz);
        RL_HIP(hipGetLastError());
    }
    // The trace units may be handed out again as soon as this returns (task_scheduler.rs:262-271): their
    // next render must not overwrite mapped_photons before the kernels above have read them.
    if (n_trace_units != 0) {
        RL_HIP(hipEventRecord(u->plotted, u->stream));
        for (uint32_t k = 0; k < n_trace_units; ++k) RL_HIP(hipStreamWaitEvent(trace_units[k]->stream, u->plotted, 0));
    }
    return RL_OK;
}

int rl_plot_unit_clear(RlPlotUnit* u) {
    if (!u) return fail(RL_E_INVALID, "null plot unit");
    int rc = use_device(u->device);
    if (rc != RL_OK) return rc;
    if ((rc = plot_settle(u)) != RL_OK) return rc; // a fused render begun into this buffer ends first
    RL_HIP(hipMemsetAsync(u->xyz, 0, (size_t)u->width * u->height * 3 * sizeof(float), u->stream));
    RL_HIP(hipEventRecord(u->cleared, u->stream)); // later fused renders wait for this
    return RL_OK;
}

int rl_plot_unit_sync(RlPlotUnit* u) {
    if (!u) return fail(RL_E_INVALID, "null plot unit");
    int rc = use_device(u->device);
    if (rc != RL_OK) return rc;
    if ((rc = plot_settle(u)) != RL_OK) return rc; // a fused render begun into this buffer ends first
    RL_HIP(hipStreamSynchronize(u->stream));
    return RL_OK;
}

int rl_plot_unit_device_buffer(RlPlotUnit* u, float** device_xyz) {
    if (!u || !device_xyz) return fail(RL_E_INVALID, "null argument");
    const int rc = plot_settle(u);
    if (rc != RL_OK) return rc;
    *device_xyz = u->xyz;
    return RL_OK;
}

int rl_plot_unit_upload(RlPlotUnit* u, const RlVector3* in) {
    if (!u || !in) return fail(RL_E_INVALID, "null argument");
    int rc = use_device(u->device);
    if (rc != RL_OK) return rc;
    if ((rc = plot_settle(u)) != RL_OK) return rc; // a fused render begun into this buffer ends first
    return upload(u->stream, {{u->xyz, in, (size_t)u->width * u->height * sizeof(RlVector3)}});
}

int rl_plot_unit_download(RlPlotUnit* u, RlVector3* out) {
    if (!u || !out) return fail(RL_E_INVALID, "null argument");
    int rc = use_device(u->device);
    if (rc != RL_OK) return rc;
    if ((rc = plot_settle(u)) != RL_OK) return rc; // a fused render begun into this buffer ends first
    return download(u->stream, {{u->xyz, out, (size_t)u->width * u->height * sizeof(RlVector3)}});
}

// ---- film for caller-supplied photons and samples (rl_plot_unit_plot_photons*, rl_plot_unit_render_samples*, rl_film.hip.h) ----
// Everything here is queued on the plot unit's own stream, whose tail is every write into the buffer so far, and the calls
// return when that stream has drained (with_film_ctx).

namespace {
// The film's constants of a launch that splats into u what it traces in `scene`.
RlFilm film_of(const RlPlotUnit* u, const RlScene* scene) {
    RlFilm film;
    film.plot = u->xyz;
    film.width = u->width;
    film.height = u->height;
    film.wm1 = (float)(int)u->width - 1.0f;
    film.hm1 = (float)(int)u->height - 1.0f;
    film.aspect_ratio = (float)u->width / (float)u->height; // plot_unit.rs:48
    film.off_cie = scene->lay.off_cie;
    return film;
}

// samples [0, n) of device arrays as paths first_path .. first_path + n - 1 (n > 0), splatted into u: one launch of the film path
// kernel on c's stream, behind the copy that zeroes the context's queue counter and writes the film's constants after it.
// `results` may be null.
int launch_film(const CallCtx& c, RlPlotUnit* u, const RlScene* scene, int fetch, const PathJob& job, uint64_t first_path,
                const RlCameraSample* samples, RlPathResult* results, uint32_t n) {
    const int rc = query_ctx_queue(c.q);
    if (rc != RL_OK) return rc;
    const RlFilmQueue fq{0, film_of(u, scene)};
    // (from pageable memory: the copy has left `fq` when the call returns)
    RL_HIP(hipMemcpyAsync(c.q->queue, &fq, sizeof fq, hipMemcpyHostToDevice, c.stream));
    return launch_persistent(c, g_film_kernels, scene, fetch, n, samples, results, n, job.seed, job.stream, first_path, job.max_segments, c.q->queue);
}

// The photon splat kernel for device array photons [0, n) (n > 0) on c's stream.
int launch_film_photons(const CallCtx& c, RlPlotUnit* u, const RlMappedPhoton* photons, uint64_t n) {
    const float aspect = (float)u->width / (float)u->height; // plot_unit.rs:48
    hipLaunchKernelGGL(rl_film_photons_kernel, dim3(grid_for(n, c.cus)), dim3(RL_BLOCK), 0, c.stream, photons, n, u->cie, u->width, u->height,
                       aspect, u->xyz);
    RL_HIP(hipGetLastError());
    return RL_OK;
}

// The light kernel with a film for the states of device array states [0, n_states) that device array list [0, n_list) names
// (n_list > 0; a null list: states 0 .. n_list - 1), splatted into u: on c's stream, the copy that zeroes the context's chunk counter
// and writes the launch's block behind it (RlLightFilmQueue), then the kernel.  `samples` and `sampled` may be null.
int launch_light_film(const CallCtx& c, RlPlotUnit* u, const RlScene* scene, int fetch, uint64_t seed, uint32_t rng_stream, const RlPathState* states,
                      uint32_t n_states, const uint32_t* list, uint32_t n_list, const RlRayHit* hits, const RlCameraSample* camera, uint8_t* sampled,
                      RlLightSample* samples) {
    const int rc = query_ctx_queue(c.q);
    if (rc != RL_OK) return rc;
    RlLightFilmQueue lq;
    std::memset(&lq, 0, sizeof lq);
    lq.job.light = light_job(scene, seed, rng_stream, states, n_states, list, n_list, hits, samples);
    lq.job.camera = camera;
    lq.job.sampled = sampled;
    lq.job.emitter_flags = scene->emitter_flags;
    lq.job.n_objects = scene->emitter_flags ? scene->lay.n_objects : 0u;
    lq.job.film = film_of(u, scene);
    // (from pageable memory: the copy has left `lq` when the call returns)
    RL_HIP(hipMemcpyAsync(c.q->queue, &lq, sizeof lq, hipMemcpyHostToDevice, c.stream));
    return launch_persistent(c, g_light_film_kernels, scene, fetch, n_list, c.q->queue);
}

int light_film_check(const RlPlotUnit* u, const RlScene* scene, int fetch, const void* states, uint32_t n_states, const void* list, uint32_t n_list,
                     const void* hits, const void* camera) {
    if (!u) return fail(RL_E_INVALID, "null plot unit");
    if (!scene) return fail(RL_E_INVALID, "null scene");
    if (fetch_check(fetch) != RL_OK) return RL_E_INVALID;
    if (n_list > 0 && (!states || !hits || !camera)) return fail(RL_E_INVALID, "null state, hit or camera sample buffer");
    return identity_list_check(list, n_list, n_states);
}

// rl_plot_unit_render_samples_direct* for device arrays camera, results [0, n) (0 < n <= RL_QUERY_CHUNK; results may be null) as
// paths first_path .. first_path + n - 1, on c's stream, which has drained on return: begin, then step / light / swap until no
// path is live or max_segments segments are made.  The working buffers are the context's: states | hits | two lists | sampled.
int direct_chunk(const CallCtx& c, RlPlotUnit* u, const RlScene* scene, int fetch, const PathJob& job, uint64_t first_path,
                 const RlCameraSample* camera, RlPathResult* results, uint32_t n) {
    int rc = device_reserve(&c.q->direct, (size_t)n * (sizeof(RlPathState) + sizeof(RlRayHit) + 2u * sizeof(uint32_t) + 1u));
    if (rc != RL_OK) return rc;
    RlPathState* states = (RlPathState*)c.q->direct.p;
    RlRayHit* hits = (RlRayHit*)(states + n);
    uint32_t* lists[2] = {(uint32_t*)(hits + n), (uint32_t*)(hits + n) + n};
    uint8_t* sampled = (uint8_t*)(lists[1] + n);
    hipLaunchKernelGGL(rl_direct_begin_kernel, dim3(grid_for(n, c.cus)), dim3(RL_BLOCK), 0, c.stream, camera, first_path, states, sampled, n);
    RL_HIP(hipGetLastError());
    const uint32_t* list = nullptr; // the first round's: every state
    uint32_t n_list = n;
    for (uint32_t segment = 0; segment < job.max_segments && n_list > 0; ++segment) {
        uint32_t n_live = 0; // (written by the step's copy, read behind the synchronise)
        uint32_t* live = lists[segment & 1u];
        if ((rc = launch_list_step(c, scene, fetch, job.seed, job.stream, 0u, states, n, list, n_list, hits, live, &n_live)) != RL_OK) return rc;
        // (the list the step was given: the states that have just ended are seen once)
        if ((rc = launch_light_film(c, u, scene, fetch, job.seed, job.stream, states, n, list, n_list, hits, camera, sampled, nullptr)) != RL_OK) return rc;
        RL_HIP(hipStreamSynchronize(c.stream));
        list = live;
        n_list = n_live;
    }
    if (results) {
        hipLaunchKernelGGL(rl_direct_results_kernel, dim3(grid_for(n, c.cus)), dim3(RL_BLOCK), 0, c.stream, (const RlPathState*)states, results, n);
        RL_HIP(hipGetLastError());
    }
    RL_HIP(hipStreamSynchronize(c.stream));
    return RL_OK;
}

// rl_plot_unit_render_direct for paths first_path .. first_path + n_paths - 1 (n_paths > 0) on c's stream: the counters behind the
// context's queue counter zeroed once, then launches of at most RL_DIRECT_LAUNCH paths back to back -- each behind the copy that
// zeroes the queue counter and writes the launch's block after it (RlDirectQueue, up to its counters) -- and the copy of the
// counters into `counters`, which holds them when the stream has drained.  `results` may be null.
#define RL_DIRECT_LAUNCH (1ull << 30)
int launch_direct(const CallCtx& c, RlPlotUnit* u, const RlScene* scene, int fetch, const PathJob& job, uint64_t first_path, uint64_t n_paths,
                  RlPathResult* results, unsigned long long* counters) {
    const int rc = query_ctx_queue(c.q);
    if (rc != RL_OK) return rc;
    RlDirectQueue* dq = (RlDirectQueue*)c.q->queue;
    RL_HIP(hipMemsetAsync(dq->stats, 0, sizeof dq->stats, c.stream));
    for (uint64_t done = 0; done < n_paths;) {
        const uint32_t k = (uint32_t)std::min<uint64_t>(n_paths - done, RL_DIRECT_LAUNCH);
        RlDirectQueue q;
        std::memset(&q, 0, sizeof q);
        q.job.results = results ? results + done : nullptr;
        q.job.emitters = scene->emitters;
        q.job.emitter_flags = scene->emitter_flags;
        q.job.seed = job.seed;
        q.job.first_path = first_path + done;
        q.job.n_paths = k;
        q.job.stream = job.stream;
        q.job.max_segments = job.max_segments;
        q.job.n_emitters = (uint32_t)scene->emitter_objects.size();
        q.job.n_objects = scene->emitter_flags ? scene->lay.n_objects : 0u;
        q.job.aspect_ratio = (float)u->width / (float)u->height; // trace_unit.rs:73, as launch_camera has it
        q.job.film = film_of(u, scene);
        // (from pageable memory: the copy has left `q` when the call returns)
        RL_HIP(hipMemcpyAsync(dq, &q, offsetof(RlDirectQueue, stats), hipMemcpyHostToDevice, c.stream));
        const int r = launch_persistent(c, g_direct_kernels, scene, fetch, k, c.q->queue);
        if (r != RL_OK) return r;
        done += k;
    }
    RL_HIP(hipMemcpyAsync(counters, dq->stats, sizeof dq->stats, hipMemcpyDeviceToHost, c.stream));
    return RL_OK;
}

int samples_check(const RlPlotUnit* u, const RlScene* scene, int fetch, uint32_t max_segments, uint64_t first_path, const void* samples,
                  uint32_t n, PathJob* job) {
    if (!u) return fail(RL_E_INVALID, "null plot unit");
    if (!scene) return fail(RL_E_INVALID, "null scene");
    if (fetch_check(fetch) != RL_OK || max_segments_resolve(max_segments, &job->max_segments) != RL_OK) return RL_E_INVALID;
    if (path_range_check(first_path, n) != RL_OK) return RL_E_INVALID;
    if (n > 0 && !samples) return fail(RL_E_INVALID, "null sample buffer");
    return RL_OK;
}
} // namespace

int rl_plot_unit_plot_photons(RlPlotUnit* u, const RlMappedPhoton* photons, uint64_t n) {
    if (!u) return fail(RL_E_INVALID, "null plot unit");
    if (n > 0 && !photons) return fail(RL_E_INVALID, "null photon buffer");
    if (n == 0) return RL_OK;
    return with_film_ctx(u, [&](const CallCtx& c) -> int {
        return staged_chunks(c, n, {staged_in(STAGING_RAYS, photons, sizeof(RlMappedPhoton))}, [&](uint64_t, uint64_t k) -> int {
            return launch_film_photons(c, u, (const RlMappedPhoton*)c.q->staging[STAGING_RAYS], k);
        });
    });
}

int rl_plot_unit_plot_photons_device(RlPlotUnit* u, const RlMappedPhoton* device_photons, uint64_t n) {
    if (!u) return fail(RL_E_INVALID, "null plot unit");
    if (n > 0 && !device_photons) return fail(RL_E_INVALID, "null photon buffer");
    if (n == 0) return RL_OK;
    return with_film_ctx(u, {"rl_plot_unit_plot_photons_device", "rl_plot_unit_plot_photons", {device_photons}},
                         [&](const CallCtx& c) -> int { return launch_film_photons(c, u, device_photons, n); });
}

int rl_plot_unit_render_samples(RlPlotUnit* u, const RlScene* scene, int primitive_fetch, uint64_t seed, uint32_t stream,
                                uint64_t first_path_index, uint32_t max_segments, const RlCameraSample* samples, uint32_t n,
                                RlPathResult* results) {
    PathJob job{seed, stream, 0u};
    const int rc = samples_check(u, scene, primitive_fetch, max_segments, first_path_index, samples, n, &job);
    if (rc != RL_OK || n == 0) return rc;
    if (scene->device != u->device) return fail(RL_E_STATE, "scene and plot unit live on different devices");
    return with_film_ctx(u, [&](const CallCtx& c) -> int {
        return staged_chunks(c, n, {staged_in(STAGING_HITS, samples, sizeof(RlCameraSample)), staged_out(STAGING_RAYS, results, sizeof(RlPathResult))},
                             [&](uint32_t first, uint32_t k) -> int {
                                 return launch_film(c, u, scene, primitive_fetch, job, first_path_index + first, (const RlCameraSample*)c.q->staging[STAGING_HITS],
                                                    results ? (RlPathResult*)c.q->staging[STAGING_RAYS] : nullptr, k);
                             });
    });
}

int rl_plot_unit_render_samples_device(RlPlotUnit* u, const RlScene* scene, int primitive_fetch, uint64_t seed, uint32_t stream,
                                       uint64_t first_path_index, uint32_t max_segments, const RlCameraSample* device_samples,
                                       uint32_t n, RlPathResult* device_results) {
    PathJob job{seed, stream, 0u};
    const int rc = samples_check(u, scene, primitive_fetch, max_segments, first_path_index, device_samples, n, &job);
    if (rc != RL_OK || n == 0) return rc;
    if (scene->device != u->device) return fail(RL_E_STATE, "scene and plot unit live on different devices");
    return with_film_ctx(u, {"rl_plot_unit_render_samples_device", "rl_plot_unit_render_samples", {device_samples, device_results}},
                         [&](const CallCtx& c) -> int {
                             return launch_film(c, u, scene, primitive_fetch, job, first_path_index, device_samples, device_results, n);
                         });
}

// (The device mismatch is reported before the early-out on an empty list.)
int rl_plot_unit_light_paths_device(RlPlotUnit* u, const RlScene* scene, int primitive_fetch, uint64_t seed, uint32_t stream,
                                    const RlPathState* device_states, uint32_t n_states, const uint32_t* device_list, uint32_t n_list,
                                    const RlRayHit* device_hits, const RlCameraSample* device_camera, uint8_t* device_sampled,
                                    RlLightSample* device_samples) {
    int rc = light_film_check(u, scene, primitive_fetch, device_states, n_states, device_list, n_list, device_hits, device_camera);
    if (rc != RL_OK) return rc;
    if (scene->device != u->device) return fail(RL_E_STATE, "scene and plot unit live on different devices");
    if (n_list == 0) return RL_OK;
    const char* what = "rl_plot_unit_light_paths_device";
    if ((rc = states_aligned(device_states, what)) != RL_OK) return rc;
    if ((rc = aligned_check(what, "the sample or camera sample buffer", 16, {device_samples, device_camera})) != RL_OK) return rc;
    if ((rc = aligned_check(what, "the list", 4, {device_list})) != RL_OK) return rc;
    return with_film_ctx(u, {what, "rl_plot_unit_light_paths", {device_states, device_hits, device_list, device_samples, device_camera, device_sampled}},
                         [&](const CallCtx& c) -> int {
                             return launch_light_film(c, u, scene, primitive_fetch, seed, stream, device_states, n_states, device_list, n_list, device_hits,
                                                      device_camera, device_sampled, device_samples);
                         });
}

// Not chunked (WholeArrays).  The caller's samples and `sampled` bytes go in too: those of the states that are not listed come back
// as they were.
int rl_plot_unit_light_paths(RlPlotUnit* u, const RlScene* scene, int primitive_fetch, uint64_t seed, uint32_t stream, const RlPathState* states,
                             uint32_t n_states, const uint32_t* list, uint32_t n_list, const RlRayHit* hits, const RlCameraSample* camera,
                             uint8_t* sampled, RlLightSample* samples) {
    int rc = light_film_check(u, scene, primitive_fetch, states, n_states, list, n_list, hits, camera);
    if (rc != RL_OK) return rc;
    if (scene->device != u->device) return fail(RL_E_STATE, "scene and plot unit live on different devices");
    if (n_list == 0 || n_states == 0) return RL_OK; // (a given list of a state buffer without states: every entry is skipped)
    if ((rc = use_device(u->device)) != RL_OK) return rc;
    Whole d_states = whole_in(states, (size_t)n_states * sizeof(RlPathState)), d_hits = whole_in(hits, (size_t)n_states * sizeof(RlRayHit));
    Whole d_camera = whole_in(camera, (size_t)n_states * sizeof(RlCameraSample)), d_samples = whole_inout(samples, (size_t)n_states * sizeof(RlLightSample));
    Whole d_sampled = whole_inout(sampled, (size_t)n_states), d_list = whole_in(list, (size_t)n_list * sizeof(uint32_t));
    WholeArrays dev(&d_states, &d_hits, &d_camera, &d_samples, &d_sampled, &d_list);
    if ((rc = dev.allocate()) != RL_OK) return rc;
    return with_film_ctx(u, [&](const CallCtx& c) -> int {
        const int r = dev.run(c.stream, [&]() -> int {
            return launch_light_film(c, u, scene, primitive_fetch, seed, stream, (const RlPathState*)d_states.dev, n_states, (const uint32_t*)d_list.dev, n_list,
                                     (const RlRayHit*)d_hits.dev, (const RlCameraSample*)d_camera.dev, (uint8_t*)d_sampled.dev, (RlLightSample*)d_samples.dev);
        });
        if (r != RL_OK) return r;
        RL_HIP(hipStreamSynchronize(c.stream)); // (the buffers are freed when the call returns)
        return RL_OK;
    });
}

int rl_plot_unit_render_samples_direct(RlPlotUnit* u, const RlScene* scene, int primitive_fetch, uint64_t seed, uint32_t stream,
                                       uint64_t first_path_index, uint32_t max_segments, const RlCameraSample* samples, uint32_t n,
                                       RlPathResult* results) {
    PathJob job{seed, stream, 0u};
    const int rc = samples_check(u, scene, primitive_fetch, max_segments, first_path_index, samples, n, &job);
    if (rc != RL_OK || n == 0) return rc;
    if (scene->device != u->device) return fail(RL_E_STATE, "scene and plot unit live on different devices");
    return with_film_ctx(u, [&](const CallCtx& c) -> int {
        return staged_chunks(c, n, {staged_in(STAGING_HITS, samples, sizeof(RlCameraSample)), staged_out(STAGING_RAYS, results, sizeof(RlPathResult))},
                             [&](uint32_t first, uint32_t k) -> int {
                                 return direct_chunk(c, u, scene, primitive_fetch, job, first_path_index + first, (const RlCameraSample*)c.q->staging[STAGING_HITS],
                                                     results ? (RlPathResult*)c.q->staging[STAGING_RAYS] : nullptr, k);
                             });
    });
}

int rl_plot_unit_render_samples_direct_device(RlPlotUnit* u, const RlScene* scene, int primitive_fetch, uint64_t seed, uint32_t stream,
                                              uint64_t first_path_index, uint32_t max_segments, const RlCameraSample* device_samples,
                                              uint32_t n, RlPathResult* device_results) {
    PathJob job{seed, stream, 0u};
    int rc = samples_check(u, scene, primitive_fetch, max_segments, first_path_index, device_samples, n, &job);
    if (rc != RL_OK || n == 0) return rc;
    if (scene->device != u->device) return fail(RL_E_STATE, "scene and plot unit live on different devices");
    const char* what = "rl_plot_unit_render_samples_direct_device";
    if ((rc = aligned_check(what, "the sample buffer", 16, {device_samples})) != RL_OK) return rc;
    return with_film_ctx(u, {what, "rl_plot_unit_render_samples_direct", {device_samples, device_results}}, [&](const CallCtx& c) -> int {
        for (uint32_t first = 0; first < n;) {
            const uint32_t k = n - first < RL_QUERY_CHUNK ? n - first : (uint32_t)RL_QUERY_CHUNK;
            const int r = direct_chunk(c, u, scene, primitive_fetch, job, first_path_index + first, device_samples + first,
                                       device_results ? device_results + first : nullptr, k);
            if (r != RL_OK) return r;
            first += k;
        }
        return RL_OK;
    });
}

int rl_plot_unit_render_direct(RlPlotUnit* u, const RlScene* scene, int primitive_fetch, uint64_t seed, uint32_t stream,
                               uint64_t first_path_index, uint64_t n_paths, uint32_t max_segments, RlPathResult* device_results,
                               RlDirectStats* stats) {
    PathJob job{seed, stream, 0u};
    if (!u) return fail(RL_E_INVALID, "null plot unit");
    if (!scene) return fail(RL_E_INVALID, "null scene");
    if (fetch_check(primitive_fetch) != RL_OK || max_segments_resolve(max_segments, &job.max_segments) != RL_OK) return RL_E_INVALID;
    if (path_range_check(first_path_index, n_paths) != RL_OK) return RL_E_INVALID;
    const char* what = "rl_plot_unit_render_direct";
    int rc = aligned_check(what, "the result buffer", 16, {device_results});
    if (rc != RL_OK) return rc;
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (n_paths == 0) return RL_OK;
    if (scene->device != u->device) return fail(RL_E_STATE, "scene and plot unit live on different devices");
    unsigned long long counters[RL_DIRECT_COUNTERS] = {};
    rc = with_film_ctx(u, {what, "rl_scene_render_rays", {device_results}}, [&](const CallCtx& c) -> int {
        return launch_direct(c, u, scene, primitive_fetch, job, first_path_index, n_paths, device_results, counters);
    });
    if (rc != RL_OK || !stats) return rc;
    stats->paths = n_paths;
    stats->segments = counters[RL_DIRECT_SEGMENTS];
    stats->light_samples = counters[RL_DIRECT_LIGHT_SAMPLES];
    stats->shadow_rays = counters[RL_DIRECT_SHADOW_RAYS];
    stats->visible = counters[RL_DIRECT_SHADOW_RAYS] - counters[RL_DIRECT_VISIBLE]; // (the kernel counts the blocked ones)
    stats->endings_kept = counters[RL_DIRECT_KEPT];
    stats->endings_dropped = counters[RL_DIRECT_DROPPED];
    return RL_OK;
}

// ---- denoising guides (rl_scene_render_features, rl_features.hip.h) ------------------------------------------------------------
namespace {
// rl_scene_render_features for paths first_path .. first_path + n_paths - 1 (n_paths > 0) on c's stream, which is the first given
// unit's: behind what is queued into the other given units (their `ready`), the counters behind the context's queue counter zeroed
// once, then launches of at most RL_FEATURE_LAUNCH paths back to back -- each behind the copy that zeroes the queue counter and
// writes the launch's block after it (RlFeatureQueue, up to its counters) -- the copy of the counters into `counters`, which
// holds them when the stream has drained, and the other given units' streams behind all of it (their `tail`).  `units` are the
// albedo, normal and aux units; any may be null, and so may `records`.
#define RL_FEATURE_LAUNCH (1ull << 30)
int launch_features(const CallCtx& c, const RlScene* scene, int fetch, const PathJob& job, uint32_t width, uint32_t height, uint64_t first_path,
                    uint64_t n_paths, RlPlotUnit* const units[3], RlFeatureSample* records, unsigned long long* counters) {
    int rc = query_ctx_queue(c.q);
    if (rc != RL_OK) return rc;
    for (int k = 0; k < 3; ++k) {
        RlPlotUnit* o = units[k];
        if (!o || o->stream == c.stream) continue;
        if ((rc = hand_over(o->ready, o->stream, c.stream)) != RL_OK) return rc; // the launches write behind what is queued into o
    }
    RlFeatureQueue* fq = (RlFeatureQueue*)c.q->queue;
    RL_HIP(hipMemsetAsync(fq->stats, 0, sizeof fq->stats, c.stream));
    for (uint64_t done = 0; done < n_paths;) {
        const uint32_t k = (uint32_t)std::min<uint64_t>(n_paths - done, RL_FEATURE_LAUNCH);
        RlFeatureQueue q;
        std::memset(&q, 0, sizeof q);
        q.job.records = records ? records + done : nullptr;
        q.job.albedo = units[0] ? units[0]->xyz : nullptr;
        q.job.normal = units[1] ? units[1]->xyz : nullptr;
        q.job.aux = units[2] ? units[2]->xyz : nullptr;
        q.job.seed = job.seed;
        q.job.first_path = first_path + done;
        q.job.n_paths = k;
        q.job.stream = job.stream;
        q.job.max_segments = job.max_segments;
        q.job.width = width;
        q.job.height = height;
        q.job.wm1 = (float)(int)width - 1.0f;
        q.job.hm1 = (float)(int)height - 1.0f;
        q.job.aspect_ratio = (float)width / (float)height; // trace_unit.rs:73 and plot_unit.rs:48, as launch_camera and film_of have it
        q.job.off_cie = scene->lay.off_cie;
        // (from pageable memory: the copy has left `q` when the call returns)
        RL_HIP(hipMemcpyAsync(fq, &q, offsetof(RlFeatureQueue, stats), hipMemcpyHostToDevice, c.stream));
        const int r = launch_persistent(c, g_feature_kernels, scene, fetch, k, c.q->queue);
        if (r != RL_OK) return r;
        done += k;
    }
    RL_HIP(hipMemcpyAsync(counters, fq->stats, sizeof fq->stats, hipMemcpyDeviceToHost, c.stream));
    for (int k = 0; k < 3; ++k) {
        RlPlotUnit* o = units[k];
        if (!o || o->stream == c.stream) continue;
        if ((rc = hand_over(o->tail, c.stream, o->stream)) != RL_OK) return rc; // o's tail covers what was written into it here
    }
    return RL_OK;
}
} // namespace

int rl_scene_render_features(const RlScene* scene, int primitive_fetch, uint32_t width, uint32_t height, uint64_t seed, uint32_t stream,
                             uint64_t first_path_index, uint64_t n_paths, uint32_t max_segments, RlPlotUnit* albedo, RlPlotUnit* normal,
                             RlPlotUnit* aux, RlFeatureSample* device_records, RlFeatureStats* stats) {
    const char* what = "rl_scene_render_features";
    PathJob job{seed, stream, 0u};
    if (!scene) return fail(RL_E_INVALID, "null scene");
    if (fetch_check(primitive_fetch) != RL_OK) return RL_E_INVALID;
    if (width == 0 || height == 0) return fail(RL_E_INVALID, std::string(what) + ": zero image size");
    if (check_image_size(what, width, height) != RL_OK) return RL_E_INVALID;
    if (max_segments_resolve(max_segments, &job.max_segments) != RL_OK) return RL_E_INVALID;
    if (max_segments == 0u) job.max_segments = RL_FEATURE_MAX_SEGMENTS;
    if (path_range_check(first_path_index, n_paths) != RL_OK) return RL_E_INVALID;
    int rc = aligned_check(what, "the record buffer", 16, {device_records});
    if (rc != RL_OK) return rc;
    RlPlotUnit* const units[3] = {albedo, normal, aux};
    if ((albedo && (albedo == normal || albedo == aux)) || (normal && normal == aux))
        return fail(RL_E_INVALID, std::string(what) + ": the albedo, normal and aux units must be distinct plot units");
    if (n_paths == 0) {
        if (stats) std::memset(stats, 0, sizeof *stats);
        return RL_OK;
    }
    RlPlotUnit* first = nullptr;
    for (RlPlotUnit* u : units) {
        if (!u) continue;
        if (u->device != scene->device) return fail(RL_E_STATE, "scene and plot unit live on different devices");
        if (u->width != width || u->height != height)
            return fail(RL_E_STATE, std::string(what) + ": a plot unit is not " + std::to_string(width) + " x " + std::to_string(height));
        if (!first) first = u;
    }
    if (stats) std::memset(stats, 0, sizeof *stats);
    for (RlPlotUnit* u : units) // a fused render begun into a given unit ends first (with_call_ctx: the first one's)
        if (u && u != first && (rc = plot_settle(u)) != RL_OK) return rc;
    unsigned long long counters[RL_FEATURE_COUNTERS] = {};
    rc = with_call_ctx(scene->device, "scene", first, {what, "no such form", {device_records}}, [&](const CallCtx& c) -> int {
        return launch_features(c, scene, primitive_fetch, job, width, height, first_path_index, n_paths, units, device_records, counters);
    });
    if (rc != RL_OK || !stats) return rc;
    stats->paths = n_paths;
    stats->segments = counters[RL_FEATURE_SEGMENTS];
    for (int k = 0; k < 4; ++k) stats->kinds[k] = counters[RL_FEATURE_KINDS + k];
    return RL_OK;
}

// ---- GatherUnit ---------------------------------------------------------------------------------

int rl_gather_unit_create(int device, uint32_t width, uint32_t height, RlGatherUnit** out) {
    RlGatherUnit* u = nullptr;
    const int rc = unit_new("gather unit", device, width, height, 1u, out, &u);
    if (rc != RL_OK) return rc;
    const size_t bytes = (size_t)width * height * 3 * sizeof(float);
    u->ledger.alloc_zeroed(&u->acc, bytes);
    u->ledger.alloc_zeroed(&u->comp, bytes);
    u->ledger.stream(&u->stream);
    return unit_created("gather unit allocation", u, rl_gather_unit_destroy, out);
}

int rl_gather_unit_destroy(RlGatherUnit* u) {
    if (!u) return RL_OK;
    (void)hipSetDevice(u->device);
    u->ledger.release();
    delete u;
    return RL_OK;
}

int rl_gather_unit_accumulate(RlGatherUnit* u, RlPlotUnit* plot) {
    if (!u || !plot) return fail(RL_E_INVALID, "null handle");
    int cus = 256;
    int rc = match_check(plot, u);
    if (rc == RL_OK) rc = enter_device(u->device, &cus);
    if (rc != RL_OK) return rc;
    if ((rc = plot_settle(plot)) != RL_OK) return rc; // a fused render begun into this buffer ends first
    const uint64_t n_floats = (uint64_t)u->width * u->height * 3;
    if ((rc = hand_over(plot->ready, plot->stream, u->stream)) != RL_OK) return rc; // everything plotted / splatted / reduced into the buffer so far
    hipLaunchKernelGGL(rl_gather_kernel, dim3(grid_for(n_floats / 4 + 1, cus)), dim3(RL_BLOCK), 0, u->stream, u->acc, u->comp,
                       plot->xyz, n_floats);
    RL_HIP(hipGetLastError());
    return hand_over(plot->cleared, u->stream, plot->stream); // the kernel also cleared the plot buffer (app.rs:147)
}

int rl_gather_unit_sync(RlGatherUnit* u) {
    if (!u) return fail(RL_E_INVALID, "null gather unit");
    int rc = use_device(u->device);
    if (rc != RL_OK) return rc;
    RL_HIP(hipStreamSynchronize(u->stream));
    return RL_OK;
}

int rl_gather_unit_download(RlGatherUnit* u, RlVector3* tristimulus, RlVector3* compensation) {
    if (!u) return fail(RL_E_INVALID, "null gather unit");
    int rc = use_device(u->device);
    if (rc != RL_OK) return rc;
    const size_t bytes = (size_t)u->width * u->height * sizeof(RlVector3);
    return download(u->stream, {{u->acc, tristimulus, bytes}, {u->comp, compensation, bytes}});
}

int rl_gather_unit_save(RlGatherUnit* u, const char* path) {
    if (!u || !path) return fail(RL_E_INVALID, "null argument");
    const size_t n = (size_t)u->width * u->height;
    std::vector<RlVector3> host(2 * n);
    int rc = rl_gather_unit_download(u, host.data(), host.data() + n);
    if (rc != RL_OK) return rc;
    FILE* f = std::fopen(path, "wb");
    if (!f) return fail(RL_E_IO, std::string("failed to open file ") + path);
    const size_t written = std::fwrite(host.data(), sizeof(RlVector3), 2 * n, f);
    const bool flushed = std::fflush(f) == 0 && fsync(fileno(f)) == 0; // on disk before a caller renames it into place (rl_app.cpp)
    const int closed = std::fclose(f);
    if (written != 2 * n || closed != 0 || !flushed) return fail(RL_E_IO, std::string("failed to write raw buffer ") + path);
    return RL_OK;
}

int rl_gather_unit_load(RlGatherUnit* u, const char* path) {
    if (!u || !path) return fail(RL_E_INVALID, "null argument");
    int rc = use_device(u->device);
    if (rc != RL_OK) return rc;
    FILE* f = std::fopen(path, "rb");
    if (!f) return fail(RL_E_IO, std::string("failed to open file ") + path);
    const size_t n = (size_t)u->width * u->height;
    std::vector<RlVector3> host(2 * n);
    // read_into semantics (read.rs:20-32): a short file leaves the tail as it was.
    if ((rc = rl_gather_unit_download(u, host.data(), host.data() + n)) != RL_OK) {
        std::fclose(f);
        return rc;
    }
    (void)std::fread(host.data(), 1, 2 * n * sizeof(RlVector3), f);
    std::fclose(f);
    return upload(u->stream, {{u->acc, host.data(), n * sizeof(RlVector3)}, {u->comp, host.data() + n, n * sizeof(RlVector3)}});
}

// ---- TonemapUnit --------------------------------------------------------------------------------

int rl_tonemap_unit_create(int device, uint32_t width, uint32_t height, RlTonemapUnit** out) {
    RlTonemapUnit* u = nullptr; // (no stream of its own: last_stream is a gather unit's)
    const int rc = unit_new("tonemap unit", device, width, height, 1u, out, &u);
    if (rc != RL_OK) return rc;
    const size_t n = (size_t)width * height * 3;
    u->ledger.alloc_zeroed(&u->rgb, n);
    u->ledger.alloc_zeroed(&u->srgb, n * sizeof(float));
    u->ledger.alloc_zeroed(&u->max_intensity, sizeof(float));
    return unit_created("tonemap unit allocation", u, rl_tonemap_unit_destroy, out);
}

int rl_tonemap_unit_destroy(RlTonemapUnit* u) {
    if (!u) return RL_OK;
    (void)hipSetDevice(u->device);
    u->ledger.release();
    delete u;
    return RL_OK;
}

int rl_tonemap_unit_tonemap(RlTonemapUnit* u, RlGatherUnit* gather) {
    if (!u || !gather) return fail(RL_E_INVALID, "null handle");
    int cus = 256;
    int rc = match_check(gather, u);
    if (rc == RL_OK) rc = enter_device(u->device, &cus);
    if (rc != RL_OK) return rc;
    const uint32_t n_pixels = u->width * u->height;
    hipLaunchKernelGGL(rl_exposure_kernel, dim3(1), dim3(RL_EXPOSURE_BLOCK), 0, gather->stream, gather->acc, n_pixels, (float)n_pixels,
                       u->max_intensity);
    RL_HIP(hipGetLastError());
    hipLaunchKernelGGL(rl_tonemap_kernel, dim3(grid_for(n_pixels, cus)), dim3(RL_BLOCK), 0, gather->stream, gather->acc, n_pixels,
                       u->max_intensity, u->rgb, u->srgb);
    RL_HIP(hipGetLastError());
    u->last_stream = gather->stream;
    return RL_OK;
}

int rl_tonemap_unit_rgb(RlTonemapUnit* u, uint8_t* out) {
    if (!u || !out) return fail(RL_E_INVALID, "null argument");
    int rc = use_device(u->device);
    if (rc != RL_OK) return rc;
    return download(u->last_stream, {{u->rgb, out, (size_t)u->width * u->height * 3}});
}

int rl_tonemap_unit_srgb_float(RlTonemapUnit* u, float* out, float* max_intensity) {
    if (!u) return fail(RL_E_INVALID, "null tonemap unit");
    int rc = use_device(u->device);
    if (rc != RL_OK) return rc;
    return download(u->last_stream, {{u->srgb, out, (size_t)u->width * u->height * 3 * sizeof(float)}, {u->max_intensity, max_intensity, sizeof(float)}});
}

// ---- DenoiseUnit (rl_denoise.hip.h) -----------------------------------------------------------------

namespace {
std::atomic<uint64_t> g_denoise_launches[2]; // rl_debug_denoise_launches: guide launches, pass launches
std::atomic<uint64_t> g_denoise_variance_launches[2]; // rl_debug_denoise_variance_launches: V_0 launches, variance pass launches
}

int rl_denoise_params_default(RlDenoiseParams* out) {
    if (!out) return fail(RL_E_INVALID, "null output");
    std::memset(out, 0, sizeof(*out));
    out->iterations = RL_DENOISE_ITERATIONS;
    out->sigma_colour = 0.6f;
    out->sigma_normal = 0.3f;
    out->sigma_depth = 0.1f;
    out->sigma_albedo = 0.2f;
    return RL_OK;
}

int rl_denoise_unit_create(int device, uint32_t width, uint32_t height, RlDenoiseUnit** out) {
    RlDenoiseUnit* u = nullptr;
    const int rc = unit_new("denoise unit", device, width, height, 1u, out, &u);
    if (rc != RL_OK) return rc;
    const size_t n = (size_t)width * height;
    u->ledger.alloc(&u->guides, n * RL_DENOISE_GUIDE_WORDS * sizeof(RlF4));
    for (float*& b : u->pingpong) u->ledger.alloc(&b, n * 3 * sizeof(float));
    for (hipEvent_t& ev : u->ready) u->ledger.event(&ev);
    for (EventPair& ep : u->timed) u->ledger.pair(&ep);
    return unit_created("denoise unit allocation", u, rl_denoise_unit_destroy, out);
}

// The unit has no stream of its own: its work runs on dst's, and rl_denoise_unit_denoise returns with that stream drained, also
// after a failure (drained), so nothing reads or writes the unit's buffers here.
int rl_denoise_unit_destroy(RlDenoiseUnit* u) {
    if (!u) return RL_OK;
    (void)hipSetDevice(u->device);
    u->ledger.release();
    delete u;
    return RL_OK;
}

int rl_denoise_variance_params_default(RlDenoiseParams* out) {
    const int rc = rl_denoise_params_default(out);
    if (rc == RL_OK) out->sigma_colour = 3.0f; // standard deviations of the luminance difference
    return rc;
}

namespace {

// Both denoise calls: `what` is the call's name; `error` non-null makes it the variance form (rl_denoise_unit_denoise_variance),
// whose null check of `error` is its caller's.  The checks and their order are the header's.
int denoise_call(const char* what, RlDenoiseUnit* u, RlGatherUnit* image, RlGatherUnit* albedo, RlGatherUnit* normal, RlGatherUnit* aux,
                 RlErrorUnit* error, const RlDenoiseParams* params, RlGatherUnit* dst, float* variance_out) {
    const std::string name = std::string(what) + ": ";
    RlDenoiseParams p;
    if (params) p = *params;
    else if (error) (void)rl_denoise_variance_params_default(&p);
    else (void)rl_denoise_params_default(&p);
    if (p.iterations > RL_DENOISE_MAX_ITERATIONS)
        return fail(RL_E_INVALID, name + "iterations " + std::to_string(p.iterations) + " above RL_DENOISE_MAX_ITERATIONS = " +
                                      std::to_string(RL_DENOISE_MAX_ITERATIONS));
    const float sigmas[4] = {p.sigma_colour, p.sigma_normal, p.sigma_depth, p.sigma_albedo};
    const char* const sigma_names[4] = {"sigma_colour", "sigma_normal", "sigma_depth", "sigma_albedo"};
    for (int k = 0; k < 4; ++k)
        if (!(sigmas[k] == 0.0f || (sigmas[k] >= 1e-3f && sigmas[k] <= 1e3f))) // (a NaN fails both)
            return fail(RL_E_INVALID, name + sigma_names[k] + " must be 0 (the term is off) or in [1e-3, 1e3]");
    if (p.reserved[0] != 0u || p.reserved[1] != 0u || p.reserved[2] != 0u) return fail(RL_E_INVALID, name + "params.reserved must be 0");
    RlGatherUnit* const given[5] = {image, albedo, normal, aux, dst};
    for (int a = 0; a < 5; ++a)
        for (int b = a + 1; b < 5; ++b)
            if (given[a] && given[a] == given[b]) return fail(RL_E_INVALID, name + "the gather units must be distinct handles");
    if (error && error->observations < 2)
        return fail(RL_E_STATE, name + std::to_string(error->observations) + " observations in the error unit: a variance needs at least 2");
    int rc = RL_OK, cus = 256;
    for (RlGatherUnit* g : given)
        if (g && (rc = match_check(g, u)) != RL_OK) return rc;
    if (error && (rc = match_check(error, u)) != RL_OK) return rc;
    if ((rc = enter_device(u->device, &cus)) != RL_OK) return rc;
    const uint32_t iterations = p.iterations ? p.iterations : RL_DENOISE_ITERATIONS;
    const uint32_t n_pixels = u->width * u->height;
    if (error && !u->variance[1]) { // the first variance call on this unit: its two planes, its event and its timed pair
        if (!u->variance[0]) RL_HIP(u->ledger.make_alloc(&u->variance[0], (size_t)n_pixels * sizeof(float)));
        if (!u->error_ready) RL_HIP(u->ledger.make_event(&u->error_ready));
        if (!u->timed_variance.start) RL_HIP(u->ledger.make_pair(&u->timed_variance));
        RL_HIP(u->ledger.make_alloc(&u->variance[1], (size_t)n_pixels * sizeof(float)));
    }
    hipStream_t stream = dst->stream;
    u->timed_passes = 0; // the pairs are re-recorded from here on: readable again once the call has completed
    if (error) u->timed_variance_done = false;
    rc = drained(stream, [&]() -> int {
        for (int k = 0; k < 4; ++k) { // everything queued on the streams of the units the call reads
            const int r = given[k] ? hand_over(u->ready[k], given[k]->stream, stream) : RL_OK;
            if (r != RL_OK) return r;
        }
        int r = error ? hand_over(u->error_ready, error->stream, stream) : RL_OK;
        if (r != RL_OK) return r;
        r = timed_launch(u->timed[0], stream, &g_denoise_launches[0], [&] {
            hipLaunchKernelGGL(rl_denoise_guides_kernel, dim3(grid_for(n_pixels, cus)), dim3(RL_BLOCK), 0, stream, albedo ? albedo->acc : nullptr,
                               normal ? normal->acc : nullptr, aux ? aux->acc : nullptr, n_pixels, u->guides);
        });
        if (r != RL_OK) return r;
        if (error) { // V_0, from the planes as everything queued on the error unit's stream leaves them
            const double n_total = (double)error->paths, ratio = n_total / (double)(error->observations - 1);
            r = timed_launch(u->timed_variance, stream, &g_denoise_variance_launches[0], [&] {
                hipLaunchKernelGGL(rl_variance_denoise_kernel, dim3(grid_for((uint64_t)n_pixels / 2 + 1, cus)), dim3(RL_BLOCK), 0, stream,
                                   (const double*)error->sum_y, (const double*)error->sum_q, (uint64_t)n_pixels, n_total, ratio, u->variance[0]);
            });
            if (r != RL_OK) return r;
        }
        // k(sigma), f32 on the host
        float k[4];
        for (int t = 0; t < 4; ++t) k[t] = sigmas[t] == 0.0f ? 0.0f : 1.0f / (sigmas[t] * sigmas[t]);
        const float* in = image->acc;
        for (uint32_t i = 0; i < iterations; ++i) {
            float* out = i + 1 == iterations ? dst->acc : u->pingpong[i & 1u];
            RlDenoisePass job;
            job.width = u->width;
            job.height = u->height;
            job.step = 1u << i;
            job.classes_x = std::min(job.step, u->width);
            job.classes_y = std::min(job.step, u->height);
            job.tiles_x = ((u->width + job.step - 1) / job.step + RL_DENOISE_TILE - 1) / RL_DENOISE_TILE;
            job.tiles_y = ((u->height + job.step - 1) / job.step + RL_DENOISE_TILE - 1) / RL_DENOISE_TILE;
            // the colour sigma halves per pass (exact); in the variance form it stays and the filtered variance shrinks instead
            job.kc = error ? k[0] : k[0] * (float)(1u << 2 * i);
            job.kn = k[1];
            job.kz = k[2];
            job.ka = k[3];
            // (at most 2^31 / 17 * 32 / 256 workgroups for any image the units accept: one grid dimension holds them)
            const uint64_t groups = (uint64_t)job.tiles_x * job.classes_x * job.tiles_y * job.classes_y;
            if (error)
                r = timed_launch(u->timed[1 + i], stream, &g_denoise_variance_launches[1], [&] {
                    hipLaunchKernelGGL(rl_variance_denoise_pass_kernel, dim3((uint32_t)groups), dim3(RL_DENOISE_TILE * RL_DENOISE_TILE), 0, stream, in,
                                       (const float*)u->variance[i & 1u], (const RlF4*)u->guides, job, out, u->variance[(i + 1u) & 1u]);
                });
            else
                r = timed_launch(u->timed[1 + i], stream, &g_denoise_launches[1], [&] {
                    hipLaunchKernelGGL(rl_denoise_pass_kernel, dim3((uint32_t)groups), dim3(RL_DENOISE_TILE * RL_DENOISE_TILE), 0, stream, in, u->guides, job, out);
                });
            if (r != RL_OK) return r;
            in = out;
        }
        RL_HIP(hipMemsetAsync(dst->comp, 0, (size_t)n_pixels * 3 * sizeof(float), stream));
        if (error && variance_out) // V_iterations, after the last pass and before the drain
            RL_HIP(hipMemcpyAsync(variance_out, u->variance[iterations & 1u], (size_t)n_pixels * sizeof(float), hipMemcpyDeviceToHost, stream));
        return RL_OK;
    }());
    if (rc == RL_OK) u->timed_passes = iterations;
    if (rc == RL_OK && error) u->timed_variance_done = true;
    return rc;
}

} // namespace

int rl_denoise_unit_denoise(RlDenoiseUnit* u, RlGatherUnit* image, RlGatherUnit* albedo, RlGatherUnit* normal, RlGatherUnit* aux,
                            const RlDenoiseParams* params, RlGatherUnit* dst) {
    if (!u || !image || !dst) return fail(RL_E_INVALID, "rl_denoise_unit_denoise: null denoise unit, image or dst");
    return denoise_call("rl_denoise_unit_denoise", u, image, albedo, normal, aux, nullptr, params, dst, nullptr);
}

int rl_denoise_unit_denoise_variance(RlDenoiseUnit* u, RlGatherUnit* image, RlGatherUnit* albedo, RlGatherUnit* normal, RlGatherUnit* aux,
                                     RlErrorUnit* error, const RlDenoiseParams* params, RlGatherUnit* dst, float* variance_out) {
    if (!u || !image || !dst || !error) return fail(RL_E_INVALID, "rl_denoise_unit_denoise_variance: null denoise unit, image, dst or error unit");
    return denoise_call("rl_denoise_unit_denoise_variance", u, image, albedo, normal, aux, error, params, dst, variance_out);
}

// ---- SpectralUnit (rl_spectral.hip.h) ---------------------------------------------------------------

namespace {
std::atomic<uint64_t> g_spectral_launches[2]; // rl_debug_spectral_launches: splat launches, project launches

int spectral_nodes_check(const char* what, uint32_t n_nodes) {
    if (n_nodes >= 2u && n_nodes <= RL_SPECTRAL_MAX_NODES) return RL_OK;
    return fail(RL_E_INVALID, std::string(what) + ": n_nodes " + std::to_string(n_nodes) + " outside 2 .. RL_SPECTRAL_MAX_NODES = " +
                                  std::to_string(RL_SPECTRAL_MAX_NODES));
}
float spectral_spacing(uint32_t n_nodes) { return 400.0f / (float)(n_nodes - 1u); }

// The splat kernel for device array photons [0, n) (n > 0) on `stream`.
int launch_spectral_photons(RlSpectralUnit* u, hipStream_t stream, int cus, const RlMappedPhoton* photons, uint64_t n) {
    const float aspect = (float)u->width / (float)u->height; // plot_unit.rs:48
    u->timed_done[0] = false; // readable again once the call has completed (spectral_drained)
    return timed_launch(u->timed[0], stream, &g_spectral_launches[0], [&] {
        hipLaunchKernelGGL(rl_spectral_photons_kernel, dim3(grid_for(n, cus)), dim3(RL_BLOCK), 0, stream, photons, n, u->width, u->height, u->n_nodes,
                           u->spacing, aspect, u->film);
    });
}

// A splat call borrows a query context (with_call_ctx: its staging buffers; its own stream stays idle) and queues everything on the
// spectral unit's stream, which has drained when the call returns, also after a failure: rc is what the call's body returned.
int spectral_drained(RlSpectralUnit* u, int rc) {
    if ((rc = drained(u->stream, rc)) == RL_OK) u->timed_done[0] = true;
    return rc;
}
} // namespace

int rl_spectral_unit_create(int device, uint32_t width, uint32_t height, uint32_t n_nodes, RlSpectralUnit** out) {
    if (!out) return fail(RL_E_INVALID, "null output handle");
    *out = nullptr;
    if (width == 0 || height == 0) return fail(RL_E_INVALID, "zero-sized spectral unit");
    int rc = spectral_nodes_check("spectral unit", n_nodes);
    if (rc != RL_OK) return rc;
    const uint64_t n_pixels = (uint64_t)width * height; // (below 2^64; times n_nodes only once it is known to be below 2^31)
    if (n_pixels > RL_MAX_PIXELS || n_pixels * n_nodes > RL_MAX_PIXELS)
        return fail(RL_E_INVALID, "spectral unit: " + std::to_string(width) + " x " + std::to_string(height) + " pixels x " + std::to_string(n_nodes) +
                                      " nodes exceed RL_MAX_PIXELS = 2^31 - 1");
    rc = use_device(device);
    if (rc != RL_OK) return rc;
    RlSpectralUnit* u = new (std::nothrow) RlSpectralUnit();
    if (!u) return fail(RL_E_INVALID, "out of host memory");
    u->device = device;
    u->width = width;
    u->height = height;
    u->n_nodes = n_nodes;
    u->spacing = spectral_spacing(n_nodes);
    u->ledger.alloc_zeroed(&u->film, (size_t)n_pixels * n_nodes * sizeof(float));
    u->ledger.alloc(&u->matrix, (size_t)RL_SPECTRAL_MAX_NODES * 3 * sizeof(float));
    u->ledger.stream(&u->stream);
    u->ledger.event(&u->ready);
    for (EventPair& ep : u->timed) u->ledger.pair(&ep);
    return unit_created("spectral unit allocation", u, rl_spectral_unit_destroy, out);
}

int rl_spectral_unit_destroy(RlSpectralUnit* u) {
    if (!u) return RL_OK;
    (void)hipSetDevice(u->device);
    u->ledger.release();
    delete u;
    return RL_OK;
}

int rl_spectral_unit_clear(RlSpectralUnit* u) {
    if (!u) return fail(RL_E_INVALID, "null spectral unit");
    int rc = use_device(u->device);
    if (rc != RL_OK) return rc;
    RL_HIP(hipMemsetAsync(u->film, 0, (size_t)u->width * u->height * u->n_nodes * sizeof(float), u->stream));
    return RL_OK;
}

int rl_spectral_unit_plot(RlSpectralUnit* u, RlTraceUnit* const* trace_units, uint32_t n_trace_units) {
    if (!u || (!trace_units && n_trace_units)) return fail(RL_E_INVALID, "null argument");
    int cus = 256;
    const int rc = enter_device(u->device, &cus);
    if (rc != RL_OK || n_trace_units == 0) return rc;
    // The splats are in the film on return, so the trace units' next renders need no event of this unit's to wait for.
    return spectral_drained(u, [&]() -> int {
        for (uint32_t k = 0; k < n_trace_units; ++k) {
            RlTraceUnit* t = trace_units[k];
            if (!t || t->device != u->device) return fail(RL_E_STATE, "trace unit missing or on another device");
            int r = render_end(t); // a render that was begun: its photons are complete after this
            if (r != RL_OK) return r;
            RL_HIP(hipStreamWaitEvent(u->stream, t->rendered, 0)); // mapped_photons complete (a no-op after a synchronous render)
            if ((r = launch_spectral_photons(u, u->stream, cus, t->photons, t->n_photons)) != RL_OK) return r;
        }
        return RL_OK;
    }());
}

int rl_spectral_unit_plot_photons(RlSpectralUnit* u, const RlMappedPhoton* photons, uint64_t n) {
    if (!u) return fail(RL_E_INVALID, "null spectral unit");
    if (n > 0 && !photons) return fail(RL_E_INVALID, "null photon buffer");
    if (n == 0) return RL_OK;
    return with_call_ctx(u->device, "spectral unit", nullptr, DeviceArrays{}, [&](const CallCtx& q) -> int {
        const CallCtx c{q.q, u->stream, q.cus};
        return spectral_drained(u, staged_chunks(c, n, {staged_in(STAGING_RAYS, photons, sizeof(RlMappedPhoton))}, [&](uint64_t, uint64_t k) -> int {
            return launch_spectral_photons(u, c.stream, c.cus, (const RlMappedPhoton*)c.q->staging[STAGING_RAYS], k);
        }));
    });
}

int rl_spectral_unit_plot_photons_device(RlSpectralUnit* u, const RlMappedPhoton* device_photons, uint64_t n) {
    if (!u) return fail(RL_E_INVALID, "null spectral unit");
    if (n > 0 && !device_photons) return fail(RL_E_INVALID, "null photon buffer");
    if (n == 0) return RL_OK;
    return with_call_ctx(u->device, "spectral unit", nullptr, {"rl_spectral_unit_plot_photons_device", "rl_spectral_unit_plot_photons", {device_photons}},
                         [&](const CallCtx& q) -> int { return spectral_drained(u, launch_spectral_photons(u, u->stream, q.cus, device_photons, n)); });
}

int rl_spectral_unit_download(RlSpectralUnit* u, float* out) {
    if (!u || !out) return fail(RL_E_INVALID, "null argument");
    int rc = use_device(u->device);
    if (rc != RL_OK) return rc;
    return download(u->stream, {{u->film, out, (size_t)u->width * u->height * u->n_nodes * sizeof(float)}});
}

int rl_spectral_unit_upload(RlSpectralUnit* u, const float* in) {
    if (!u || !in) return fail(RL_E_INVALID, "null argument");
    int rc = use_device(u->device);
    if (rc != RL_OK) return rc;
    return upload(u->stream, {{u->film, in, (size_t)u->width * u->height * u->n_nodes * sizeof(float)}});
}

int rl_spectral_unit_project(RlSpectralUnit* u, const float* matrix, RlGatherUnit* dst) {
    if (!u || !matrix || !dst) return fail(RL_E_INVALID, "rl_spectral_unit_project: null spectral unit, matrix or dst");
    int cus = 256;
    int rc = match_check(dst, u);
    if (rc == RL_OK) rc = enter_device(u->device, &cus);
    if (rc != RL_OK) return rc;
    const uint64_t n_pixels = (uint64_t)u->width * u->height;
    hipStream_t stream = dst->stream;
    // (the copy reads the caller's matrix and the kernel the unit's buffers: neither outlives the call, also after a failure)
    rc = drained(stream, [&]() -> int {
        int r = hand_over(u->ready, u->stream, stream); // everything queued on the film (a clear; the splats have drained)
        if (r != RL_OK) return r;
        RL_HIP(hipMemcpyAsync(u->matrix, matrix, (size_t)u->n_nodes * 3 * sizeof(float), hipMemcpyHostToDevice, stream));
        u->timed_done[1] = false; // readable again once the call has completed
        r = timed_launch(u->timed[1], stream, &g_spectral_launches[1], [&] {
            hipLaunchKernelGGL(rl_spectral_project_kernel, dim3(grid_for(n_pixels, cus)), dim3(RL_BLOCK), 0, stream, (const float*)u->film,
                               (const float*)u->matrix, n_pixels, u->n_nodes, dst->acc);
        });
        if (r != RL_OK) return r;
        RL_HIP(hipMemsetAsync(dst->comp, 0, (size_t)n_pixels * 3 * sizeof(float), stream));
        return RL_OK;
    }());
    if (rc == RL_OK) u->timed_done[1] = true;
    return rc;
}

int rl_spectral_observer_cie1931(uint32_t n_nodes, float* out) {
    if (!out) return fail(RL_E_INVALID, "null output");
    const int rc = spectral_nodes_check("rl_spectral_observer_cie1931", n_nodes);
    if (rc != RL_OK) return rc;
    RlF4 table[RL_CIE_SAMPLES];
    std::memcpy(table, RL_CIE1931_XYZ0, sizeof table);
    const float spacing = spectral_spacing(n_nodes);
    for (uint32_t b = 0; b < n_nodes; ++b) {
        const RlF3 c = rl_tristimulus(table, 380.0f + (float)b * spacing);
        out[3u * b] = c.x;
        out[3u * b + 1u] = c.y;
        out[3u * b + 2u] = c.z;
    }
    return RL_OK;
}

// ---- GlareUnit (rl_glare.hip.h) --------------------------------------------------------------------

namespace {
std::atomic<uint64_t> g_glare_launches; // rl_debug_glare_launches: launches of rl_glare_kernel, either form

int glare_taps_check(const char* what, uint32_t taps) {
    if ((taps & 1u) && taps <= RL_GLARE_MAX_TAPS) return RL_OK;
    return fail(RL_E_INVALID, std::string(what) + ": taps " + std::to_string(taps) + " is not odd and in 1 .. RL_GLARE_MAX_TAPS = " +
                                  std::to_string(RL_GLARE_MAX_TAPS));
}
bool glare_finite(double v) { return std::fabs(v) < (double)INFINITY; }
} // namespace

int rl_glare_unit_create(int device, uint32_t width, uint32_t height, uint32_t n_nodes, uint32_t taps, RlGlareUnit** out) {
    if (!out) return fail(RL_E_INVALID, "null output handle");
    *out = nullptr;
    if (width == 0 || height == 0) return fail(RL_E_INVALID, "zero-sized glare unit");
    int rc = spectral_nodes_check("glare unit", n_nodes);
    if (rc == RL_OK) rc = glare_taps_check("glare unit", taps);
    if (rc != RL_OK) return rc;
    const uint64_t n_pixels = (uint64_t)width * height; // (below 2^64; times n_nodes only once it is known to be below 2^31)
    if (n_pixels > RL_MAX_PIXELS || n_pixels * n_nodes > RL_MAX_PIXELS)
        return fail(RL_E_INVALID, "glare unit: " + std::to_string(width) + " x " + std::to_string(height) + " pixels x " + std::to_string(n_nodes) +
                                      " nodes exceed RL_MAX_PIXELS = 2^31 - 1");
    rc = use_device(device);
    if (rc != RL_OK) return rc;
    RlGlareUnit* u = new (std::nothrow) RlGlareUnit();
    if (!u) return fail(RL_E_INVALID, "out of host memory");
    u->device = device;
    u->width = width;
    u->height = height;
    u->n_nodes = n_nodes;
    u->taps = taps;
    u->ledger.alloc(&u->tables, (size_t)n_nodes * taps * taps * sizeof(float));
    u->ledger.alloc(&u->matrix, (size_t)n_nodes * 3 * sizeof(float));
    u->ledger.stream(&u->stream);
    u->ledger.event(&u->ready);
    u->ledger.pair(&u->timed);
    return unit_created("glare unit allocation", u, rl_glare_unit_destroy, out);
}

int rl_glare_unit_destroy(RlGlareUnit* u) {
    if (!u) return RL_OK;
    (void)hipSetDevice(u->device);
    u->ledger.release();
    delete u;
    return RL_OK;
}

int rl_glare_unit_set_kernels(RlGlareUnit* u, const float* tables) {
    if (!u || !tables) return fail(RL_E_INVALID, "rl_glare_unit_set_kernels: null glare unit or tables");
    const int rc = use_device(u->device);
    if (rc != RL_OK) return rc;
    const size_t n = (size_t)u->n_nodes * u->taps * u->taps;
    bool finite = true;
    for (size_t k = 0; k < n && finite; ++k) finite = std::fabs(tables[k]) < INFINITY;
    // (the copy reads the caller's tables: it has run when the call returns, also after a failure)
    const int copied = drained(u->stream, [&]() -> int {
        RL_HIP(hipMemcpyAsync(u->tables, tables, n * sizeof(float), hipMemcpyHostToDevice, u->stream));
        return RL_OK;
    }());
    if (copied != RL_OK) return copied;
    u->exact_skip = !finite;
    u->has_tables = 1u;
    return RL_OK;
}

int rl_glare_unit_apply(RlGlareUnit* u, RlSpectralUnit* film, const float* matrix, RlGatherUnit* dst) {
    if (!u || !film || !matrix || !dst) return fail(RL_E_INVALID, "rl_glare_unit_apply: null glare unit, film, matrix or dst");
    if (!u->has_tables) return fail(RL_E_STATE, "the glare unit has no tables: call rl_glare_unit_set_kernels first");
    int cus = 256;
    int rc = match_check(film, u);
    if (rc == RL_OK && film->n_nodes != u->n_nodes)
        rc = fail(RL_E_STATE, "spectral unit does not match the glare unit: " + std::to_string(film->n_nodes) + " nodes against " +
                                  std::to_string(u->n_nodes));
    if (rc == RL_OK) rc = match_check(dst, u);
    if (rc == RL_OK) rc = enter_device(u->device, &cus);
    if (rc != RL_OK) return rc;
    const uint64_t n_pixels = (uint64_t)u->width * u->height;
    const uint32_t tiles_x = (u->width + RL_GLARE_TILE_X - 1u) / RL_GLARE_TILE_X; // (at most 2^25 and 2^27: the sums cannot wrap)
    const uint32_t tiles_y = (u->height + RL_GLARE_TILE_Y - 1u) / RL_GLARE_TILE_Y;
    const uint64_t n_tiles = (uint64_t)tiles_x * tiles_y;                          // (at most ~2^31 / 1024 + 2^27 + 2^25)
    const unsigned grid = (unsigned)std::min<uint64_t>(n_tiles, RL_GLARE_MAX_GRID);
    const size_t lds = (size_t)rl_glare_lds_floats(u->taps) * sizeof(float);
    hipStream_t stream = dst->stream;
    // (the copy reads the caller's matrix and the kernel the units' buffers: neither outlives the call, also after a failure)
    rc = drained(stream, [&]() -> int {
        int r = hand_over(film->ready, film->stream, stream); // everything queued on the film (a clear; the splats have drained)
        if (r == RL_OK) r = hand_over(u->ready, u->stream, stream); // ... and on the unit: its tables
        if (r != RL_OK) return r;
        RL_HIP(hipMemcpyAsync(u->matrix, matrix, (size_t)u->n_nodes * 3 * sizeof(float), hipMemcpyHostToDevice, stream));
        u->timed_done = false; // readable again once the call has completed
        r = timed_launch(u->timed, stream, &g_glare_launches, [&] {
            if (u->exact_skip)
                hipLaunchKernelGGL(rl_glare_kernel<true>, dim3(grid), dim3(RL_GLARE_BLOCK), lds, stream, (const float*)film->film, (const float*)u->tables,
                                   (const float*)u->matrix, u->width, u->height, u->n_nodes, u->taps, tiles_x, (uint32_t)n_tiles, dst->acc);
            else
                hipLaunchKernelGGL(rl_glare_kernel<false>, dim3(grid), dim3(RL_GLARE_BLOCK), lds, stream, (const float*)film->film, (const float*)u->tables,
                                   (const float*)u->matrix, u->width, u->height, u->n_nodes, u->taps, tiles_x, (uint32_t)n_tiles, dst->acc);
        });
        if (r != RL_OK) return r;
        RL_HIP(hipMemsetAsync(dst->comp, 0, (size_t)n_pixels * 3 * sizeof(float), stream));
        return RL_OK;
    }());
    if (rc == RL_OK) u->timed_done = true;
    return rc;
}

int rl_glare_psf_veil(uint32_t taps, double r0, float* out) {
    if (!out) return fail(RL_E_INVALID, "null output");
    const int rc = glare_taps_check("rl_glare_psf_veil", taps);
    if (rc != RL_OK) return rc;
    if (!(glare_finite(r0) && r0 > 0.0)) return fail(RL_E_INVALID, "rl_glare_psf_veil: r0 is not finite and greater than 0");
    const int radius = (int)(taps >> 1);
    for (int j = 0; j < (int)taps; ++j)
        for (int i = 0; i < (int)taps; ++i) {
            const double d2 = (double)((i - radius) * (i - radius) + (j - radius) * (j - radius));
            const double q = 1.0 + d2 / (r0 * r0);
            out[(size_t)j * taps + i] = (float)(1.0 / (q * std::sqrt(q)));
        }
    return RL_OK;
}

int rl_glare_kernels_scaled(const float* psf, uint32_t psf_taps, double lambda0, uint32_t n_nodes, double strength, uint32_t taps, float* out) {
    if (!psf || !out) return fail(RL_E_INVALID, "rl_glare_kernels_scaled: null psf or output");
    if (!(psf_taps & 1u) || psf_taps > 257u)
        return fail(RL_E_INVALID, "rl_glare_kernels_scaled: psf_taps " + std::to_string(psf_taps) + " is not odd and in 1 .. 257");
    if (!(glare_finite(lambda0) && lambda0 > 0.0)) return fail(RL_E_INVALID, "rl_glare_kernels_scaled: lambda0 is not finite and greater than 0");
    int rc = spectral_nodes_check("rl_glare_kernels_scaled", n_nodes);
    if (rc != RL_OK) return rc;
    if (!(strength >= 0.0 && strength <= 1.0)) return fail(RL_E_INVALID, "rl_glare_kernels_scaled: strength is outside 0 .. 1");
    if ((rc = glare_taps_check("rl_glare_kernels_scaled", taps)) != RL_OK) return rc;
    for (size_t k = 0; k < (size_t)psf_taps * psf_taps; ++k)
        if (!(psf[k] >= 0.0f && psf[k] < INFINITY))
            return fail(RL_E_INVALID, "rl_glare_kernels_scaled: psf entry " + std::to_string(k) + " is not finite and at least 0");
    const double size = (double)psf_taps, radius_in = (double)(psf_taps >> 1);
    const int radius = (int)(taps >> 1);
    // p = 0 outside the base table; whether (ix, iy) is inside is decided on the doubles, before any conversion to int
    auto at = [&](double ix, double iy) -> double {
        if (!(ix >= 0.0 && ix < size && iy >= 0.0 && iy < size)) return 0.0;
        return (double)psf[(size_t)iy * psf_taps + (size_t)ix];
    };
    std::vector<double> w((size_t)taps * taps);
    std::vector<float> result((size_t)n_nodes * taps * taps);
    for (uint32_t b = 0; b < n_nodes; ++b) {
        const double lambda = 380.0 + (double)b * (400.0 / (double)(n_nodes - 1u));
        const double s = lambda / lambda0;
        double sum = 0.0;
        for (int j = 0; j < (int)taps; ++j)
            for (int i = 0; i < (int)taps; ++i) {
                const double pu = -(double)(i - radius) / s + radius_in, pv = -(double)(j - radius) / s + radius_in;
                const double iu = std::floor(pu), iv = std::floor(pv);
                const double fu = pu - iu, fv = pv - iv;
                const double p00 = at(iu, iv), p10 = at(iu + 1.0, iv), p01 = at(iu, iv + 1.0), p11 = at(iu + 1.0, iv + 1.0);
                const double v = ((1.0 - fu) * p00 + fu * p10) * (1.0 - fv) + ((1.0 - fu) * p01 + fu * p11) * fv;
                w[(size_t)j * taps + i] = v;
                sum = sum + v;
            }
        if (!(sum > 0.0))
            return fail(RL_E_INVALID, "rl_glare_kernels_scaled: the psf gives node " + std::to_string(b) + " nothing (the sum of its table is not > 0)");
        for (int j = 0; j < (int)taps; ++j)
            for (int i = 0; i < (int)taps; ++i) {
                double t = strength * (w[(size_t)j * taps + i] / sum);
                if (i == radius && j == radius) t = t + (1.0 - strength);
                result[((size_t)b * taps + j) * taps + i] = (float)t;
            }
    }
    std::memcpy(out, result.data(), result.size() * sizeof(float));
    return RL_OK;
}

// ---- RelightUnit (rl_relight.hip.h) ----------------------------------------------------------------

namespace {
std::atomic<uint64_t> g_relight_launches[3]; // rl_debug_relight_launches: splat launches, path launches, mix launches

size_t relight_planes(const RlRelightUnit* u) { return (size_t)u->n_groups * u->n_nodes; }
size_t relight_film_bytes(const RlRelightUnit* u) { return (size_t)u->width * u->height * relight_planes(u) * sizeof(float); }

// The routed splat for device arrays samples, results [0, n) (n > 0; the unit has a table) on `stream`.
int launch_relight_splat(RlRelightUnit* u, hipStream_t stream, int cus, const RlCameraSample* samples, const RlPathResult* results, uint64_t n) {
    const float aspect = (float)u->width / (float)u->height; // plot_unit.rs:48, as launch_spectral_photons has it
    u->timed_done[0] = false; // readable again once the call has completed (relight_drained)
    return timed_launch(u->timed[0], stream, &g_relight_launches[0], [&] {
        hipLaunchKernelGGL(rl_relight_splat_kernel, dim3(grid_for(n, cus)), dim3(RL_BLOCK), 0, stream, samples, results, n, (const uint8_t*)u->groups,
                           u->n_objects, u->width, u->height, u->n_nodes, u->n_groups, u->spacing, aspect, u->film);
    });
}

// As spectral_drained: a splat or render call queues everything on the unit's stream, which has drained when the call returns.
int relight_drained(RlRelightUnit* u, int rc) {
    if ((rc = drained(u->stream, rc)) == RL_OK) u->timed_done[0] = true;
    return rc;
}

// What the two forms of rl_relight_unit_plot_results check before any device work, in the header's order.
int relight_results_check(const RlRelightUnit* u, const void* samples, const void* results, uint64_t n) {
    if (!u) return fail(RL_E_INVALID, "null relight unit");
    if (n > 0 && (!samples || !results)) return fail(RL_E_INVALID, "null sample or result buffer");
    if (u->n_objects == 0u) return fail(RL_E_STATE, "the relight unit has no table: call rl_relight_unit_set_groups first");
    return RL_OK;
}

bool relight_positive(float v) { return v > 0.0f && v < INFINITY; }
} // namespace

int rl_relight_unit_create(int device, uint32_t width, uint32_t height, uint32_t n_nodes, uint32_t n_groups, RlRelightUnit** out) {
    if (!out) return fail(RL_E_INVALID, "null output handle");
    *out = nullptr;
    if (width == 0 || height == 0) return fail(RL_E_INVALID, "zero-sized relight unit");
    int rc = spectral_nodes_check("relight unit", n_nodes);
    if (rc != RL_OK) return rc;
    if (n_groups < 1u || n_groups > RL_RELIGHT_MAX_GROUPS)
        return fail(RL_E_INVALID, "relight unit: n_groups " + std::to_string(n_groups) + " outside 1 .. RL_RELIGHT_MAX_GROUPS = " +
                                      std::to_string(RL_RELIGHT_MAX_GROUPS));
    const uint64_t n_pixels = (uint64_t)width * height; // (below 2^64; times the planes, at most 16 * 401, only once it is known to be below 2^31)
    if (n_pixels > RL_MAX_PIXELS || n_pixels * n_nodes * n_groups > RL_MAX_PIXELS)
        return fail(RL_E_INVALID, "relight unit: " + std::to_string(width) + " x " + std::to_string(height) + " pixels x " + std::to_string(n_nodes) +
                                      " nodes x " + std::to_string(n_groups) + " groups exceed RL_MAX_PIXELS = 2^31 - 1");
    rc = use_device(device);
    if (rc != RL_OK) return rc;
    RlRelightUnit* u = new (std::nothrow) RlRelightUnit();
    if (!u) return fail(RL_E_INVALID, "out of host memory");
    u->device = device;
    u->width = width;
    u->height = height;
    u->n_nodes = n_nodes;
    u->n_groups = n_groups;
    u->spacing = spectral_spacing(n_nodes);
    u->ledger.alloc_zeroed(&u->film, relight_film_bytes(u));
    u->ledger.alloc(&u->matrix, relight_planes(u) * 3 * sizeof(float));
    u->ledger.stream(&u->stream);
    u->ledger.event(&u->ready);
    for (EventPair& ep : u->timed) u->ledger.pair(&ep);
    return unit_created("relight unit allocation", u, rl_relight_unit_destroy, out);
}

int rl_relight_unit_destroy(RlRelightUnit* u) {
    if (!u) return RL_OK;
    (void)hipSetDevice(u->device);
    u->ledger.release();
    delete u;
    return RL_OK;
}

int rl_relight_unit_clear(RlRelightUnit* u) {
    if (!u) return fail(RL_E_INVALID, "null relight unit");
    int rc = use_device(u->device);
    if (rc != RL_OK) return rc;
    RL_HIP(hipMemsetAsync(u->film, 0, relight_film_bytes(u), u->stream));
    return RL_OK;
}

int rl_relight_unit_set_groups(RlRelightUnit* u, const uint8_t* groups, uint32_t n_objects) {
    if (!u || !groups) return fail(RL_E_INVALID, "rl_relight_unit_set_groups: null relight unit or table");
    if (n_objects == 0u) return fail(RL_E_INVALID, "rl_relight_unit_set_groups: n_objects is 0");
    for (uint32_t o = 0; o < n_objects; ++o)
        if (groups[o] >= u->n_groups && groups[o] != RL_RELIGHT_DROP)
            return fail(RL_E_INVALID, "rl_relight_unit_set_groups: object " + std::to_string(o) + " has group " + std::to_string(groups[o]) +
                                          ", which is neither below n_groups = " + std::to_string(u->n_groups) + " nor RL_RELIGHT_DROP");
    int rc = use_device(u->device);
    if (rc != RL_OK) return rc;
    if (n_objects > u->groups_room) {
        // (a table that outgrows its buffer gets one of at least twice the size; the ledger keeps the old one until the unit goes)
        uint64_t room = 1024;
        while (room < n_objects) room *= 2;
        uint8_t* grown = nullptr;
        RL_HIP(u->ledger.make_alloc(&grown, (size_t)room));
        u->groups = grown;
        u->groups_room = (uint32_t)std::min<uint64_t>(room, 0xffffffffull);
    }
    u->n_objects = 0u; // (a failed copy leaves no table)
    if ((rc = upload(u->stream, {{u->groups, groups, (size_t)n_objects}})) != RL_OK) return rc;
    u->n_objects = n_objects;
    return RL_OK;
}

int rl_relight_unit_plot_results(RlRelightUnit* u, const RlCameraSample* samples, const RlPathResult* results, uint64_t n) {
    const int rc = relight_results_check(u, samples, results, n);
    if (rc != RL_OK || n == 0) return rc;
    return with_call_ctx(u->device, "relight unit", nullptr, DeviceArrays{}, [&](const CallCtx& q) -> int {
        const CallCtx c{q.q, u->stream, q.cus};
        return relight_drained(u, staged_chunks(c, n, {staged_in(STAGING_HITS, samples, sizeof(RlCameraSample)), staged_in(STAGING_RAYS, results, sizeof(RlPathResult))},
                                                [&](uint64_t, uint64_t k) -> int {
            return launch_relight_splat(u, c.stream, c.cus, (const RlCameraSample*)c.q->staging[STAGING_HITS], (const RlPathResult*)c.q->staging[STAGING_RAYS], k);
        }));
    });
}

int rl_relight_unit_plot_results_device(RlRelightUnit* u, const RlCameraSample* device_samples, const RlPathResult* device_results, uint64_t n) {
    const int rc = relight_results_check(u, device_samples, device_results, n);
    if (rc != RL_OK || n == 0) return rc;
    return with_call_ctx(u->device, "relight unit", nullptr, {"rl_relight_unit_plot_results_device", "rl_relight_unit_plot_results", {device_samples, device_results}},
                         [&](const CallCtx& q) -> int { return relight_drained(u, launch_relight_splat(u, u->stream, q.cus, device_samples, device_results, n)); });
}

int rl_relight_unit_render(RlRelightUnit* u, const RlScene* scene, int primitive_fetch, uint64_t seed, uint32_t stream, uint64_t first_path_index,
                           uint64_t n_paths, uint32_t max_segments) {
    PathJob job{seed, stream, 0u};
    if (!u) return fail(RL_E_INVALID, "null relight unit");
    if (!scene) return fail(RL_E_INVALID, "null scene");
    if (fetch_check(primitive_fetch) != RL_OK || max_segments_resolve(max_segments, &job.max_segments) != RL_OK) return RL_E_INVALID;
    if (u->n_objects == 0u) return fail(RL_E_STATE, "the relight unit has no table: call rl_relight_unit_set_groups first");
    if (path_range_check(first_path_index, n_paths) != RL_OK) return RL_E_INVALID;
    if (u->n_objects != scene->lay.n_objects)
        return fail(RL_E_STATE, "the relight unit's table has " + std::to_string(u->n_objects) + " objects and the scene " + std::to_string(scene->lay.n_objects));
    if (scene->device != u->device) return fail(RL_E_STATE, "scene and relight unit live on different devices");
    if (n_paths == 0) return RL_OK;
    int rc = use_device(u->device);
    if (rc != RL_OK) return rc;
    if (!u->samples) RL_HIP(u->ledger.make_alloc(&u->samples, (size_t)RL_QUERY_CHUNK * sizeof(RlCameraSample)));
    if (!u->rays) RL_HIP(u->ledger.make_alloc(&u->rays, (size_t)RL_QUERY_CHUNK * sizeof(RlSpectralRay)));
    if (!u->results) RL_HIP(u->ledger.make_alloc(&u->results, (size_t)RL_QUERY_CHUNK * sizeof(RlPathResult)));
    u->timed_done[1] = false;
    rc = with_call_ctx(u->device, "relight unit", nullptr, DeviceArrays{}, [&](const CallCtx& q) -> int {
        const CallCtx c{q.q, u->stream, q.cus}; // (the context lends its queue counter; its own stream stays idle)
        return relight_drained(u, [&]() -> int {
            // (the chunks share the scratch: the stream keeps them in order)
            for (uint64_t done = 0; done < n_paths;) {
                const uint32_t k = (uint32_t)std::min<uint64_t>(n_paths - done, RL_QUERY_CHUNK);
                int r = launch_camera(c, scene, u->width, u->height, seed, stream, first_path_index + done, u->samples, k);
                if (r != RL_OK) return r;
                hipLaunchKernelGGL(rl_relight_rays_kernel, dim3(grid_for(k, c.cus)), dim3(RL_BLOCK), 0, c.stream, (const RlCameraSample*)u->samples, u->rays,
                                   (uint64_t)k);
                RL_HIP(hipGetLastError());
                RL_HIP(hipEventRecord(u->timed[1].start, c.stream));
                if ((r = launch_paths(c, scene, primitive_fetch, job, first_path_index + done, u->rays, u->results, k)) != RL_OK) return r;
                RL_HIP(hipEventRecord(u->timed[1].stop, c.stream));
                g_relight_launches[1].fetch_add(1, std::memory_order_relaxed);
                if ((r = launch_relight_splat(u, c.stream, c.cus, u->samples, u->results, k)) != RL_OK) return r;
                done += k;
            }
            return RL_OK;
        }());
    });
    if (rc == RL_OK) u->timed_done[1] = true;
    return rc;
}

int rl_relight_unit_download(RlRelightUnit* u, float* out) {
    if (!u || !out) return fail(RL_E_INVALID, "null argument");
    int rc = use_device(u->device);
    if (rc != RL_OK) return rc;
    return download(u->stream, {{u->film, out, relight_film_bytes(u)}});
}

int rl_relight_unit_upload(RlRelightUnit* u, const float* in) {
    if (!u || !in) return fail(RL_E_INVALID, "null argument");
    int rc = use_device(u->device);
    if (rc != RL_OK) return rc;
    return upload(u->stream, {{u->film, in, relight_film_bytes(u)}});
}

int rl_relight_unit_mix(RlRelightUnit* u, const float* gains, const float* matrix, RlGatherUnit* dst) {
    if (!u || !matrix || !dst) return fail(RL_E_INVALID, "rl_relight_unit_mix: null relight unit, matrix or dst");
    int cus = 256;
    int rc = match_check(dst, u);
    if (rc == RL_OK) rc = enter_device(u->device, &cus);
    if (rc != RL_OK) return rc;
    // The composed matrix: row q = g * n_nodes + b is row b of the observer times that plane's gain, one f32 multiply each.
    const uint32_t planes = (uint32_t)relight_planes(u);
    std::vector<float> composed((size_t)planes * 3);
    for (uint32_t q = 0; q < planes; ++q)
        for (uint32_t k = 0; k < 3u; ++k) {
            const float m = matrix[3u * (q % u->n_nodes) + k];
            composed[3u * q + k] = gains ? gains[q] * m : m;
        }
    const uint64_t n_pixels = (uint64_t)u->width * u->height;
    hipStream_t stream = dst->stream;
    // (the copy reads `composed` and the kernel the unit's buffers: neither outlives the call, also after a failure)
    rc = drained(stream, [&]() -> int {
        int r = hand_over(u->ready, u->stream, stream); // everything queued on the film (a clear; the splats have drained)
        if (r != RL_OK) return r;
        RL_HIP(hipMemcpyAsync(u->matrix, composed.data(), composed.size() * sizeof(float), hipMemcpyHostToDevice, stream));
        u->timed_done[2] = false; // readable again once the call has completed
        // rl_spectral_project_kernel as it is: the cubes are one film of n_groups * n_nodes planes under the composed matrix
        r = timed_launch(u->timed[2], stream, &g_relight_launches[2], [&] {
            hipLaunchKernelGGL(rl_spectral_project_kernel, dim3(grid_for(n_pixels, cus)), dim3(RL_BLOCK), 0, stream, (const float*)u->film,
                               (const float*)u->matrix, n_pixels, planes, dst->acc);
        });
        if (r != RL_OK) return r;
        RL_HIP(hipMemsetAsync(dst->comp, 0, (size_t)n_pixels * 3 * sizeof(float), stream));
        return RL_OK;
    }());
    if (rc == RL_OK) u->timed_done[2] = true;
    return rc;
}

int rl_relight_gains_black_body(uint32_t n_nodes, float kelvins_from, float intensity_from, float kelvins_to, float intensity_to, float* out) {
    if (!out) return fail(RL_E_INVALID, "null output");
    const int rc = spectral_nodes_check("rl_relight_gains_black_body", n_nodes);
    if (rc != RL_OK) return rc;
    if (!relight_positive(kelvins_from) || !relight_positive(intensity_from) || !relight_positive(kelvins_to) || !relight_positive(intensity_to))
        return fail(RL_E_INVALID, "rl_relight_gains_black_body: kelvins and intensity must be finite and greater than 0");
    const float norm_from = rl_black_body_normalisation(kelvins_from, intensity_from), norm_to = rl_black_body_normalisation(kelvins_to, intensity_to);
    const float spacing = spectral_spacing(n_nodes);
    for (uint32_t b = 0; b < n_nodes; ++b) {
        const float l = 380.0f + (float)b * spacing;
        const float from = (float)rl_boltzmann((double)l, (double)kelvins_from) * norm_from; // get_intensity, material.rs:101-105
        const float to = (float)rl_boltzmann((double)l, (double)kelvins_to) * norm_to;
        out[b] = from == 0.0f ? 0.0f : to / from; // (a light that deposited nothing at this node)
    }
    return RL_OK;
}

// ---- ErrorUnit (rl_error.hip.h) ------------------------------------------------------------------

namespace {
std::atomic<uint64_t> g_error_launches[2]; // rl_debug_error_launches: observe launches, estimate launches

// The host part of an estimate (rl_error_unit_estimate, rl_robust_unit_estimate): RlErrorStats from the tiles' {t_se, t_y} pairs,
// every sum sequential in f64 in tile raster order, as the header states it.
void error_host_stats(const std::vector<double>& pairs, uint32_t tiles_x, uint32_t tiles_y, uint64_t observations, uint64_t paths,
                      RlErrorStats* stats) {
    const size_t n_tiles = (size_t)tiles_x * tiles_y;
    std::memset(stats, 0, sizeof *stats);
    stats->observations = observations;
    stats->paths = paths;
    stats->tiles_x = tiles_x;
    stats->tiles_y = tiles_y;
    double sum_se = 0.0, sum_y = 0.0;
    for (size_t i = 0; i < n_tiles; ++i) {
        sum_se = sum_se + pairs[2 * i];
        sum_y = sum_y + pairs[2 * i + 1];
    }
    stats->sum_se = sum_se;
    stats->sum_y = sum_y;
    stats->relative_error = sum_se / sum_y;
    const double m = sum_y / (double)n_tiles;
    for (size_t i = 0; i < n_tiles; ++i) {
        const double t_se = pairs[2 * i], t_y = pairs[2 * i + 1];
        const double rel = t_se / (t_y > m ? t_y : m);
        if (i == 0 || rel > stats->worst_tile_error) {
            stats->worst_tile_error = rel;
            stats->worst_tile_x = (uint32_t)(i % tiles_x);
            stats->worst_tile_y = (uint32_t)(i / tiles_x);
        }
    }
}
}

int rl_error_unit_create(int device, uint32_t width, uint32_t height, RlErrorUnit** out) {
    RlErrorUnit* u = nullptr;
    const int rc = unit_new("error unit", device, width, height, 1u, out, &u);
    if (rc != RL_OK) return rc;
    u->tiles_x = (width + RL_ERROR_TILE - 1u) / RL_ERROR_TILE;
    u->tiles_y = (height + RL_ERROR_TILE - 1u) / RL_ERROR_TILE;
    const size_t n_pixels = (size_t)width * height, n_tiles = (size_t)u->tiles_x * u->tiles_y;
    u->ledger.alloc_zeroed(&u->sum_y, n_pixels * sizeof(double));
    u->ledger.alloc_zeroed(&u->sum_q, n_pixels * sizeof(double));
    u->ledger.alloc(&u->se, n_pixels * sizeof(float));
    u->ledger.alloc(&u->tiles, n_tiles * 2 * sizeof(double));
    u->ledger.stream(&u->stream);
    u->ledger.event(&u->observed);
    for (EventPair& ep : u->timed) u->ledger.pair(&ep);
    return unit_created("error unit allocation", u, rl_error_unit_destroy, out);
}

int rl_error_unit_destroy(RlErrorUnit* u) {
    if (!u) return RL_OK;
    (void)hipSetDevice(u->device);
    u->ledger.release();
    delete u;
    return RL_OK;
}

int rl_error_unit_clear(RlErrorUnit* u) {
    if (!u) return fail(RL_E_INVALID, "null error unit");
    int rc = use_device(u->device);
    if (rc != RL_OK) return rc;
    const size_t bytes = (size_t)u->width * u->height * sizeof(double);
    RL_HIP(hipMemsetAsync(u->sum_y, 0, bytes, u->stream));
    RL_HIP(hipMemsetAsync(u->sum_q, 0, bytes, u->stream));
    u->observations = u->paths = 0;
    return RL_OK;
}

int rl_error_unit_observe(RlErrorUnit* u, RlPlotUnit* plot, uint64_t n_paths) {
    if (!u || !plot) return fail(RL_E_INVALID, "rl_error_unit_observe: null error unit or plot unit");
    if (n_paths == 0) return fail(RL_E_INVALID, "rl_error_unit_observe: n_paths is 0: an observation is the sum over at least one path");
    if (u->paths + n_paths < u->paths) return fail(RL_E_INVALID, "rl_error_unit_observe: the number of paths N overflows 64 bits");
    int cus = 256;
    int rc = match_check(plot, u);
    if (rc == RL_OK) rc = enter_device(u->device, &cus);
    if (rc != RL_OK) return rc;
    if ((rc = plot_settle(plot)) != RL_OK) return rc; // a fused render begun into this buffer ends first
    const uint64_t n_pixels = (uint64_t)u->width * u->height;
    if ((rc = hand_over(plot->ready, plot->stream, u->stream)) != RL_OK) return rc; // everything plotted / splatted / reduced into the buffer so far
    rc = timed_launch(u->timed[0], u->stream, &g_error_launches[0], [&] {
        hipLaunchKernelGGL(rl_error_observe_kernel, dim3(grid_for(n_pixels / 2 + 1, cus)), dim3(RL_BLOCK), 0, u->stream, u->sum_y, u->sum_q,
                           (const float*)plot->xyz, n_pixels, (double)n_paths);
    });
    if (rc != RL_OK) return rc;
    u->timed_done[0] = true; // recorded: rl_debug_error_ms waits for the launch itself
    if ((rc = hand_over(u->observed, u->stream, plot->stream)) != RL_OK) return rc; // a later clear or gather of the buffer must not overtake the read
    u->observations += 1;
    u->paths += n_paths;
    return RL_OK;
}

int rl_error_unit_estimate(RlErrorUnit* u, RlErrorStats* stats, float* se, double* tiles) {
    if (!u || !stats) return fail(RL_E_INVALID, "rl_error_unit_estimate: null error unit or stats");
    if (u->observations < 2)
        return fail(RL_E_STATE, "rl_error_unit_estimate: " + std::to_string(u->observations) + " observations: the estimate needs at least 2");
    int rc = use_device(u->device);
    if (rc != RL_OK) return rc;
    const size_t n_pixels = (size_t)u->width * u->height, n_tiles = (size_t)u->tiles_x * u->tiles_y;
    std::vector<double> pairs(2 * n_tiles);
    const double n_total = (double)u->paths, ratio = n_total / (double)(u->observations - 1);
    // (the copies write `pairs` and the caller's `se`: neither may be written after the call, also after a failure)
    rc = drained(u->stream, [&]() -> int {
        const int r = timed_launch(u->timed[1], u->stream, &g_error_launches[1], [&] {
            hipLaunchKernelGGL(rl_error_estimate_kernel, dim3((unsigned)n_tiles), dim3(RL_ERROR_TILE_PIXELS), 0, u->stream, (const double*)u->sum_y,
                               (const double*)u->sum_q, u->width, u->height, u->tiles_x, n_total, ratio, u->se, u->tiles);
        });
        if (r != RL_OK) return r;
        u->timed_done[1] = true; // recorded: rl_debug_error_ms waits for the launch itself
        RL_HIP(hipMemcpyAsync(pairs.data(), u->tiles, pairs.size() * sizeof(double), hipMemcpyDeviceToHost, u->stream));
        if (se) RL_HIP(hipMemcpyAsync(se, u->se, n_pixels * sizeof(float), hipMemcpyDeviceToHost, u->stream));
        return RL_OK;
    }());
    if (rc != RL_OK) return rc;
    error_host_stats(pairs, u->tiles_x, u->tiles_y, u->observations, u->paths, stats);
    if (tiles) std::memcpy(tiles, pairs.data(), pairs.size() * sizeof(double));
    return RL_OK;
}

int rl_error_unit_download(RlErrorUnit* u, double* sum_y, double* sum_q, uint64_t* observations, uint64_t* paths) {
    if (!u) return fail(RL_E_INVALID, "null error unit");
    int rc = use_device(u->device);
    if (rc != RL_OK) return rc;
    const size_t bytes = (size_t)u->width * u->height * sizeof(double);
    if ((rc = download(u->stream, {{u->sum_y, sum_y, bytes}, {u->sum_q, sum_q, bytes}})) != RL_OK) return rc;
    if (observations) *observations = u->observations;
    if (paths) *paths = u->paths;
    return RL_OK;
}

int rl_error_unit_upload(RlErrorUnit* u, const double* sum_y, const double* sum_q, uint64_t observations, uint64_t paths) {
    if (!u || !sum_y || !sum_q) return fail(RL_E_INVALID, "rl_error_unit_upload: null error unit or plane");
    int rc = use_device(u->device);
    if (rc != RL_OK) return rc;
    const size_t bytes = (size_t)u->width * u->height * sizeof(double);
    if ((rc = upload(u->stream, {{u->sum_y, sum_y, bytes}, {u->sum_q, sum_q, bytes}})) != RL_OK) return rc;
    u->observations = observations;
    u->paths = paths;
    return RL_OK;
}

// ---- RobustUnit (rl_robust.hip.h) ----------------------------------------------------------------

namespace {
std::atomic<uint64_t> g_robust_launches[2]; // rl_debug_robust_launches: observe launches, resolve launches
std::atomic<uint64_t> g_robust_estimate_launches; // rl_debug_robust_estimate_launches

size_t robust_planes_bytes(const RlRobustUnit* u) { return (size_t)u->n_buckets * 3 * u->stride * sizeof(double); }

// The sum of the buckets' path counts; false if it overflows 64 bits.
bool robust_total(const uint64_t* bucket_paths, uint32_t n_buckets, uint64_t* total) {
    uint64_t n = 0;
    for (uint32_t j = 0; j < n_buckets; ++j) {
        if (n + bucket_paths[j] < n) return false;
        n += bucket_paths[j];
    }
    *total = n;
    return true;
}
}

int rl_robust_params_default(RlRobustParams* out) {
    if (!out) return fail(RL_E_INVALID, "null output");
    out->gain = 1.0;
    out->max_trim = 0xffffffffu;
    out->reserved = 0;
    return RL_OK;
}

int rl_robust_unit_create(int device, uint32_t width, uint32_t height, uint32_t n_buckets, RlRobustUnit** out) {
    if (!out) return fail(RL_E_INVALID, "null output handle");
    *out = nullptr;
    if (width == 0 || height == 0) return fail(RL_E_INVALID, "zero-sized robust unit");
    int rc = check_image_size("robust unit", width, height);
    if (rc != RL_OK) return rc;
    if (n_buckets < 3 || n_buckets > RL_ROBUST_MAX_BUCKETS)
        return fail(RL_E_INVALID, "robust unit: n_buckets " + std::to_string(n_buckets) + " outside 3 .. RL_ROBUST_MAX_BUCKETS = " +
                                      std::to_string(RL_ROBUST_MAX_BUCKETS));
    RlRobustUnit* u = nullptr;
    if ((rc = unit_new("robust unit", device, width, height, n_buckets, out, &u)) != RL_OK) return rc;
    u->n_buckets = n_buckets;
    const size_t n_pixels = (size_t)width * height;
    u->stride = (n_pixels + 1) & ~(uint64_t)1;
    u->ledger.alloc_zeroed(&u->sums, robust_planes_bytes(u));
    u->ledger.alloc(&u->trim, n_pixels);
    u->tiles_x = (width + RL_ERROR_TILE - 1u) / RL_ERROR_TILE;
    u->tiles_y = (height + RL_ERROR_TILE - 1u) / RL_ERROR_TILE;
    u->ledger.alloc(&u->se, n_pixels * sizeof(float));
    u->ledger.alloc(&u->tiles, (size_t)u->tiles_x * u->tiles_y * 2 * sizeof(double));
    u->ledger.stream(&u->stream);
    u->ledger.event(&u->observed);
    u->ledger.event(&u->ready);
    for (EventPair& ep : u->timed) u->ledger.pair(&ep);
    u->ledger.pair(&u->timed_estimate);
    return unit_created("robust unit allocation", u, rl_robust_unit_destroy, out);
}

int rl_robust_unit_destroy(RlRobustUnit* u) {
    if (!u) return RL_OK;
    (void)hipSetDevice(u->device);
    u->ledger.release();
    delete u;
    return RL_OK;
}

int rl_robust_unit_clear(RlRobustUnit* u) {
    if (!u) return fail(RL_E_INVALID, "null robust unit");
    int rc = use_device(u->device);
    if (rc != RL_OK) return rc;
    RL_HIP(hipMemsetAsync(u->sums, 0, robust_planes_bytes(u), u->stream));
    for (uint64_t& n : u->bucket_paths) n = 0;
    u->observations = 0;
    return RL_OK;
}

int rl_robust_unit_observe(RlRobustUnit* u, RlPlotUnit* plot, uint64_t n_paths, uint32_t bucket) {
    if (!u || !plot) return fail(RL_E_INVALID, "rl_robust_unit_observe: null robust unit or plot unit");
    if (n_paths == 0) return fail(RL_E_INVALID, "rl_robust_unit_observe: n_paths is 0: an observation is the sum over at least one path");
    if (bucket >= u->n_buckets && bucket != RL_ROBUST_NEXT)
        return fail(RL_E_INVALID, "rl_robust_unit_observe: bucket " + std::to_string(bucket) + " of " + std::to_string(u->n_buckets) +
                                      " (RL_ROBUST_NEXT takes them in turn)");
    const uint32_t j = bucket == RL_ROBUST_NEXT ? (uint32_t)(u->observations % u->n_buckets) : bucket;
    uint64_t total = 0;
    if (u->bucket_paths[j] + n_paths < u->bucket_paths[j] || !robust_total(u->bucket_paths, u->n_buckets, &total) || total + n_paths < total)
        return fail(RL_E_INVALID, "rl_robust_unit_observe: the number of paths of a bucket or their total N overflows 64 bits");
    int cus = 256;
    int rc = match_check(plot, u);
    if (rc == RL_OK) rc = enter_device(u->device, &cus);
    if (rc != RL_OK) return rc;
    if ((rc = plot_settle(plot)) != RL_OK) return rc; // a fused render begun into this buffer ends first
    const uint64_t n_pixels = (uint64_t)u->width * u->height;
    if ((rc = hand_over(plot->ready, plot->stream, u->stream)) != RL_OK) return rc; // everything plotted / splatted / reduced into the buffer so far
    rc = timed_launch(u->timed[0], u->stream, &g_robust_launches[0], [&] {
        hipLaunchKernelGGL(rl_robust_observe_kernel, dim3(grid_for(n_pixels / 2 + 1, cus)), dim3(RL_BLOCK), 0, u->stream,
                           u->sums + (uint64_t)j * 3 * u->stride, (const float*)plot->xyz, n_pixels, u->stride);
    });
    if (rc != RL_OK) return rc;
    u->timed_done[0] = true; // recorded: rl_debug_robust_ms waits for the launch itself
    if ((rc = hand_over(u->observed, u->stream, plot->stream)) != RL_OK) return rc; // a later clear or gather of the buffer must not overtake the read
    u->observations += 1;
    u->bucket_paths[j] += n_paths;
    return RL_OK;
}

int rl_robust_unit_resolve(RlRobustUnit* u, const RlRobustParams* params, RlGatherUnit* dst, RlRobustStats* stats, uint8_t* trim) {
    if (!u || !params || !dst) return fail(RL_E_INVALID, "rl_robust_unit_resolve: null robust unit, params or dst");
    if (!(params->gain >= 0.0)) return fail(RL_E_INVALID, "rl_robust_unit_resolve: gain is negative or not a number");
    for (uint32_t j = 0; j < u->n_buckets; ++j)
        if (u->bucket_paths[j] == 0)
            return fail(RL_E_STATE, "rl_robust_unit_resolve: bucket " + std::to_string(j) + " holds no paths: every bucket needs an observation");
    int cus = 256;
    int rc = match_check(dst, u);
    if (rc == RL_OK) rc = enter_device(u->device, &cus);
    if (rc != RL_OK) return rc;
    const uint64_t n_pixels = (uint64_t)u->width * u->height;
    const uint32_t M = u->n_buckets, cmax = std::min(params->max_trim, (M - 1u) / 2u);
    uint64_t total = 0;
    if (!robust_total(u->bucket_paths, M, &total)) return fail(RL_E_STATE, "rl_robust_unit_resolve: the number of paths N overflows 64 bits");
    RlRobustCounts counts;
    for (uint32_t j = 0; j < RL_ROBUST_MAX_BUCKETS; ++j) counts.n[j] = j < M ? (double)u->bucket_paths[j] : 1.0;
    // one wave per workgroup (rl_robust.hip.h); as many lanes in flight as grid_for gives a streaming kernel
    const uint64_t blocks = std::min<uint64_t>((n_pixels + RL_ROBUST_LANES - 1) / RL_ROBUST_LANES, (uint64_t)cus * 8 * (RL_BLOCK / RL_ROBUST_LANES));
    const size_t lds = (size_t)M * RL_ROBUST_LANES * (3 * sizeof(double) + 1);
    std::vector<uint8_t> bytes((stats || trim) ? (size_t)n_pixels : 0);
    hipStream_t stream = dst->stream;
    u->timed_done[1] = false; // readable again once the call has completed
    // (the copy writes `bytes` and the kernel reads the unit's planes: neither outlives the call, also after a failure)
    rc = drained(stream, [&]() -> int {
        int r = hand_over(u->ready, u->stream, stream); // everything queued on the unit: clears and observations
        if (r != RL_OK) return r;
        r = timed_launch(u->timed[1], stream, &g_robust_launches[1], [&] {
            hipLaunchKernelGGL(rl_robust_resolve_kernel, dim3((unsigned)blocks), dim3(RL_ROBUST_LANES), lds, stream, (const double*)u->sums, u->stride,
                               n_pixels, M, counts, (double)total, params->gain, cmax, dst->acc, u->trim);
        });
        if (r != RL_OK) return r;
        RL_HIP(hipMemsetAsync(dst->comp, 0, (size_t)n_pixels * 3 * sizeof(float), stream));
        if (!bytes.empty()) RL_HIP(hipMemcpyAsync(bytes.data(), u->trim, (size_t)n_pixels, hipMemcpyDeviceToHost, stream));
        return RL_OK;
    }());
    if (rc != RL_OK) return rc;
    u->timed_done[1] = true;
    if (stats) {
        std::memset(stats, 0, sizeof *stats);
        stats->observations = u->observations;
        stats->paths = total;
        stats->buckets = M;
        for (const uint8_t b : bytes) {
            const uint32_t c = b & 0x7fu;
            stats->largest_trim = std::max(stats->largest_trim, c);
            stats->trimmed_pixels += c > 0 ? 1 : 0;
            stats->trimmed_buckets += 2 * c;
            stats->untrimmable_pixels += b >> 7;
        }
    }
    if (trim)
        for (size_t p = 0; p < bytes.size(); ++p) trim[p] = bytes[p] & 0x7fu;
    return RL_OK;
}

int rl_robust_unit_estimate(RlRobustUnit* u, const RlRobustParams* params, RlErrorStats* stats, float* se, double* tiles, uint8_t* trim) {
    if (!u || !params || !stats) return fail(RL_E_INVALID, "rl_robust_unit_estimate: null robust unit, params or stats");
    if (!(params->gain >= 0.0)) return fail(RL_E_INVALID, "rl_robust_unit_estimate: gain is negative or not a number");
    for (uint32_t j = 0; j < u->n_buckets; ++j)
        if (u->bucket_paths[j] == 0)
            return fail(RL_E_STATE, "rl_robust_unit_estimate: bucket " + std::to_string(j) + " holds no paths: every bucket needs an observation");
    const uint32_t M = u->n_buckets, cmax = std::min(params->max_trim, (M - 2u) / 2u); // at least two buckets are kept
    uint64_t total = 0;
    if (!robust_total(u->bucket_paths, M, &total)) return fail(RL_E_STATE, "rl_robust_unit_estimate: the number of paths N overflows 64 bits");
    int rc = use_device(u->device);
    if (rc != RL_OK) return rc;
    const size_t n_pixels = (size_t)u->width * u->height, n_tiles = (size_t)u->tiles_x * u->tiles_y;
    RlRobustCounts counts;
    for (uint32_t j = 0; j < RL_ROBUST_MAX_BUCKETS; ++j) counts.n[j] = j < M ? (double)u->bucket_paths[j] : 1.0;
    const size_t lds = (size_t)M * RL_ERROR_TILE_PIXELS * (sizeof(double) + 1); // the keys and the rank bytes (rl_robust.hip.h)
    std::vector<double> pairs(2 * n_tiles);
    // (the copies write `pairs` and the caller's `se` and `trim`: none may be written after the call, also after a failure)
    rc = drained(u->stream, [&]() -> int {
        const int r = timed_launch(u->timed_estimate, u->stream, &g_robust_estimate_launches, [&] {
            hipLaunchKernelGGL(rl_robust_estimate_kernel, dim3((unsigned)n_tiles), dim3(RL_ERROR_TILE_PIXELS), lds, u->stream, (const double*)u->sums,
                               u->stride, u->width, u->height, u->tiles_x, M, counts, (double)total, params->gain, cmax, u->se, u->tiles, u->trim);
        });
        if (r != RL_OK) return r;
        u->timed_estimate_done = true; // recorded: rl_debug_robust_estimate_ms waits for the launch itself
        RL_HIP(hipMemcpyAsync(pairs.data(), u->tiles, pairs.size() * sizeof(double), hipMemcpyDeviceToHost, u->stream));
        if (se) RL_HIP(hipMemcpyAsync(se, u->se, n_pixels * sizeof(float), hipMemcpyDeviceToHost, u->stream));
        if (trim) RL_HIP(hipMemcpyAsync(trim, u->trim, n_pixels, hipMemcpyDeviceToHost, u->stream));
        return RL_OK;
    }());
    if (rc != RL_OK) return rc;
    error_host_stats(pairs, u->tiles_x, u->tiles_y, u->observations, total, stats);
    if (tiles) std::memcpy(tiles, pairs.data(), pairs.size() * sizeof(double));
    return RL_OK;
}

int rl_robust_unit_download(RlRobustUnit* u, double* sums, uint64_t* bucket_paths, uint64_t* observations) {
    if (!u) return fail(RL_E_INVALID, "null robust unit");
    int rc = use_device(u->device);
    if (rc != RL_OK) return rc;
    const size_t n_pixels = (size_t)u->width * u->height;
    RL_HIP(hipStreamSynchronize(u->stream));
    if (sums)
        for (size_t k = 0; k < (size_t)u->n_buckets * 3; ++k) // plane by plane: the device's planes are an even number of doubles apart
            RL_HIP(hipMemcpy(sums + k * n_pixels, u->sums + k * u->stride, n_pixels * sizeof(double), hipMemcpyDeviceToHost));
    if (bucket_paths) std::memcpy(bucket_paths, u->bucket_paths, u->n_buckets * sizeof(uint64_t));
    if (observations) *observations = u->observations;
    return RL_OK;
}

int rl_robust_unit_upload(RlRobustUnit* u, const double* sums, const uint64_t* bucket_paths, uint64_t observations) {
    if (!u || !sums || !bucket_paths) return fail(RL_E_INVALID, "rl_robust_unit_upload: null robust unit, sums or bucket_paths");
    uint64_t filled = 0, total = 0;
    for (uint32_t j = 0; j < u->n_buckets; ++j) filled += bucket_paths[j] != 0 ? 1 : 0;
    if (observations < filled)
        return fail(RL_E_INVALID, "rl_robust_unit_upload: " + std::to_string(observations) + " observations cannot have filled " + std::to_string(filled) +
                                      " buckets");
    if (!robust_total(bucket_paths, u->n_buckets, &total)) return fail(RL_E_INVALID, "rl_robust_unit_upload: the number of paths N overflows 64 bits");
    int rc = use_device(u->device);
    if (rc != RL_OK) return rc;
    const size_t n_pixels = (size_t)u->width * u->height;
    RL_HIP(hipStreamSynchronize(u->stream));
    for (size_t k = 0; k < (size_t)u->n_buckets * 3; ++k)
        RL_HIP(hipMemcpy(u->sums + k * u->stride, sums + k * n_pixels, n_pixels * sizeof(double), hipMemcpyHostToDevice));
    RL_HIP(hipStreamSynchronize(nullptr)); // (the null stream only: a resident open trace kernel of another unit is not waited for)
    for (uint32_t j = 0; j < RL_ROBUST_MAX_BUCKETS; ++j) u->bucket_paths[j] = j < u->n_buckets ? bucket_paths[j] : 0;
    u->observations = observations;
    return RL_OK;
}

// ---- AdaptiveUnit (rl_adaptive_plan.h, rl_adaptive.hip.h) ----------------------------------------

namespace {
std::atomic<uint64_t> g_adaptive_launches[3]; // rl_debug_adaptive_launches: sample, path and splat launches

RlAdaptivePlan adaptive_plan_of(const RlAdaptiveUnit* u) {
    RlAdaptivePlan plan;
    plan.off = u->off;
    plan.cells = u->cells;
    plan.weight_bits = u->weight_bits;
    plan.n_tiles = u->tiles_x * u->tiles_y;
    plan.wm1 = (float)(int)u->width - 1.0f; // as film_of has them
    plan.hm1 = (float)(int)u->height - 1.0f;
    plan.aspect_ratio = (float)u->width / (float)u->height; // trace_unit.rs:73, as launch_camera has it
    return plan;
}

// The sample kernel for samples first_sample .. first_sample + n - 1 of u's plan (n > 0, inside the plan) into device array
// `samples`, and their rays into `rays` if given, on c's stream.
void launch_adaptive_samples(const CallCtx& c, const RlAdaptiveUnit* u, const RlScene* scene, uint64_t seed, uint32_t stream, uint64_t first_path,
                             uint32_t first_sample, RlCameraSample* samples, RlSpectralRay* rays, uint32_t n) {
    hipLaunchKernelGGL(rl_adaptive_samples_kernel, dim3(grid_for(n, c.cus)), dim3(RL_BLOCK), 0, c.stream, scene->blob, scene->lay,
                       adaptive_plan_of(u), seed, stream, first_path, first_sample, samples, rays, n);
    g_adaptive_launches[0].fetch_add(1, std::memory_order_relaxed);
}

int adaptive_samples_check(const RlAdaptiveUnit* u, const RlScene* scene, uint64_t first_path, uint64_t first_sample, uint32_t n, const void* out) {
    if (!u) return fail(RL_E_INVALID, "null adaptive unit");
    if (!scene) return fail(RL_E_INVALID, "null scene");
    if (n > 0 && !out) return fail(RL_E_INVALID, "null sample buffer");
    if (!u->planned) return fail(RL_E_STATE, "the adaptive unit has no plan: call rl_adaptive_unit_plan first");
    if (first_sample > u->n_paths || (uint64_t)n > u->n_paths - first_sample)
        return fail(RL_E_INVALID, "samples past the end of the plan: first_sample + n exceeds its " + std::to_string(u->n_paths) + " paths");
    if (path_range_check(first_path, first_sample + n) != RL_OK) return RL_E_INVALID;
    if (scene->device != u->device) return fail(RL_E_STATE, "scene and adaptive unit live on different devices");
    return RL_OK;
}
} // namespace

int rl_adaptive_unit_create(int device, uint32_t width, uint32_t height, RlAdaptiveUnit** out) {
    if (out && (width < 2 || height < 2)) {
        *out = nullptr;
        return fail(RL_E_INVALID, "adaptive unit: width and height must be at least 2 (a 1-wide film has no area)");
    }
    RlAdaptiveUnit* u = nullptr;
    const int rc = unit_new("adaptive unit", device, width, height, 1u, out, &u);
    if (rc != RL_OK) return rc;
    u->tiles_x = (width + RL_ERROR_TILE - 1u) / RL_ERROR_TILE;
    u->tiles_y = (height + RL_ERROR_TILE - 1u) / RL_ERROR_TILE;
    const size_t n_tiles = (size_t)u->tiles_x * u->tiles_y;
    u->ledger.alloc(&u->off, (n_tiles + 1) * sizeof(uint32_t));
    u->ledger.alloc(&u->cells, n_tiles * sizeof(RlAdaptiveCell));
    u->ledger.alloc(&u->weight_bits, n_tiles * sizeof(uint32_t));
    for (EventPair& ep : u->timed) u->ledger.pair(&ep);
    return unit_created("adaptive unit allocation", u, rl_adaptive_unit_destroy, out);
}

int rl_adaptive_unit_destroy(RlAdaptiveUnit* u) {
    if (!u) return RL_OK;
    (void)hipSetDevice(u->device);
    u->ledger.release();
    delete u;
    return RL_OK;
}

int rl_adaptive_unit_plan(RlAdaptiveUnit* u, const double* importance, double uniform_share, uint64_t n_paths, RlAdaptiveStats* stats) {
    if (!u) return fail(RL_E_INVALID, "null adaptive unit");
    if (!(uniform_share > 0.0 && uniform_share <= 1.0)) return fail(RL_E_INVALID, "rl_adaptive_unit_plan: uniform_share must be in (0, 1]");
    if (n_paths == 0 || n_paths > 0xffffffffull) return fail(RL_E_INVALID, "rl_adaptive_unit_plan: n_paths must be 1 .. 2^32 - 1");
    const size_t n_tiles = (size_t)u->tiles_x * u->tiles_y;
    std::vector<uint32_t> counts(n_tiles), off(n_tiles + 1);
    std::vector<float> weights(n_tiles);
    std::vector<RlAdaptiveCell> cells(n_tiles);
    double g_sum = 0.0;
    switch (rl_adaptive_plan_rule(u->width, u->height, importance, uniform_share, n_paths, counts.data(), weights.data(), cells.data(), &g_sum)) {
    case RL_PLAN_OK: break;
    case RL_PLAN_OVERFLOW: return fail(RL_E_INVALID, "rl_adaptive_unit_plan: the sum of the importance overflows");
    case RL_PLAN_EMPTY_TILE:
        return fail(RL_E_INVALID, "rl_adaptive_unit_plan: a tile would get no sample (a biased image): more paths or a larger uniform_share");
    default: return fail(RL_E_INVALID, "rl_adaptive_unit_plan: the shares do not sum to 1");
    }
    int rc = use_device(u->device);
    if (rc != RL_OK) return rc;
    uint64_t sum = 0; // (every prefix is below n_paths <= 2^32 - 1)
    for (size_t t = 0; t < n_tiles; ++t) off[t] = (uint32_t)sum, sum += counts[t];
    off[n_tiles] = (uint32_t)sum;
    u->planned = false; // (a failed upload leaves no plan)
    static_assert(sizeof(float) == sizeof(uint32_t), "the weights travel as their bits");
    if ((rc = upload(nullptr, {{u->off, off.data(), off.size() * sizeof(uint32_t)},
                               {u->cells, cells.data(), cells.size() * sizeof(RlAdaptiveCell)},
                               {u->weight_bits, weights.data(), weights.size() * sizeof(float)}})) != RL_OK)
        return rc;
    u->planned = true;
    u->n_paths = n_paths;
    if (stats) {
        std::memset(stats, 0, sizeof *stats);
        stats->n_paths = n_paths;
        stats->tiles_x = u->tiles_x;
        stats->tiles_y = u->tiles_y;
        stats->min_count = *std::min_element(counts.begin(), counts.end());
        stats->max_count = *std::max_element(counts.begin(), counts.end());
        stats->min_weight = *std::min_element(weights.begin(), weights.end());
        stats->max_weight = *std::max_element(weights.begin(), weights.end());
        stats->importance_sum = g_sum;
    }
    return RL_OK;
}

int rl_adaptive_unit_download_plan(RlAdaptiveUnit* u, uint32_t* counts, float* weights) {
    if (!u) return fail(RL_E_INVALID, "null adaptive unit");
    if (!u->planned) return fail(RL_E_STATE, "the adaptive unit has no plan: call rl_adaptive_unit_plan first");
    int rc = use_device(u->device);
    if (rc != RL_OK) return rc;
    const size_t n_tiles = (size_t)u->tiles_x * u->tiles_y;
    std::vector<uint32_t> off(counts ? n_tiles + 1 : 0);
    if ((rc = download(nullptr, {{u->off, counts ? off.data() : nullptr, off.size() * sizeof(uint32_t)},
                                 {u->weight_bits, weights, n_tiles * sizeof(float)}})) != RL_OK)
        return rc;
    if (counts) {
        for (size_t t = 0; t + 1 < n_tiles; ++t) counts[t] = off[t + 1] - off[t];
        counts[n_tiles - 1] = (uint32_t)(u->n_paths - off[n_tiles - 1]);
    }
    return RL_OK;
}

int rl_adaptive_unit_samples(RlAdaptiveUnit* u, const RlScene* scene, uint64_t seed, uint32_t stream, uint64_t first_path_index,
                             uint64_t first_sample, uint32_t n, RlCameraSample* out) {
    const int rc = adaptive_samples_check(u, scene, first_path_index, first_sample, n, out);
    if (rc != RL_OK || n == 0) return rc;
    return with_query_ctx(scene, [&](const CallCtx& c) -> int {
        return staged_chunks(c, n, {staged_out(STAGING_HITS, out, sizeof(RlCameraSample))}, [&](uint32_t first, uint32_t k) -> int {
            launch_adaptive_samples(c, u, scene, seed, stream, first_path_index, (uint32_t)(first_sample + first),
                                    (RlCameraSample*)c.q->staging[STAGING_HITS], nullptr, k);
            RL_HIP(hipGetLastError());
            return RL_OK;
        });
    });
}

int rl_adaptive_unit_samples_device(RlAdaptiveUnit* u, const RlScene* scene, uint64_t seed, uint32_t stream, uint64_t first_path_index,
                                    uint64_t first_sample, uint32_t n, RlCameraSample* device_out) {
    const int rc = adaptive_samples_check(u, scene, first_path_index, first_sample, n, device_out);
    if (rc != RL_OK || n == 0) return rc;
    if (aligned_check("rl_adaptive_unit_samples_device", "the sample buffer", 16, {device_out}) != RL_OK) return RL_E_INVALID;
    return with_query_ctx(scene, {"rl_adaptive_unit_samples_device", "rl_adaptive_unit_samples", {device_out}}, [&](const CallCtx& c) -> int {
        launch_adaptive_samples(c, u, scene, seed, stream, first_path_index, (uint32_t)first_sample, device_out, nullptr, n);
        RL_HIP(hipGetLastError());
        return RL_OK;
    });
}

int rl_plot_unit_render_adaptive(RlPlotUnit* plot, RlAdaptiveUnit* u, const RlScene* scene, int primitive_fetch, uint64_t seed,
                                 uint32_t stream, uint64_t first_path_index, uint32_t max_segments) {
    PathJob job{seed, stream, 0u};
    if (!plot) return fail(RL_E_INVALID, "null plot unit");
    if (!u) return fail(RL_E_INVALID, "null adaptive unit");
    if (!scene) return fail(RL_E_INVALID, "null scene");
    if (fetch_check(primitive_fetch) != RL_OK || max_segments_resolve(max_segments, &job.max_segments) != RL_OK) return RL_E_INVALID;
    if (!u->planned) return fail(RL_E_STATE, "the adaptive unit has no plan: call rl_adaptive_unit_plan first");
    if (path_range_check(first_path_index, u->n_paths) != RL_OK) return RL_E_INVALID;
    int rc = match_check(u, plot);
    if (rc != RL_OK) return rc;
    if (scene->device != plot->device) return fail(RL_E_STATE, "scene and plot unit live on different devices");
    if ((rc = use_device(u->device)) != RL_OK) return rc;
    if (!u->samples) RL_HIP(u->ledger.make_alloc(&u->samples, (size_t)RL_QUERY_CHUNK * sizeof(RlCameraSample)));
    if (!u->rays) RL_HIP(u->ledger.make_alloc(&u->rays, (size_t)RL_QUERY_CHUNK * sizeof(RlSpectralRay)));
    if (!u->results) RL_HIP(u->ledger.make_alloc(&u->results, (size_t)RL_QUERY_CHUNK * sizeof(RlPathResult)));
    u->timed_done = false;
    rc = with_film_ctx(plot, [&](const CallCtx& c) -> int {
        const float aspect = (float)plot->width / (float)plot->height; // plot_unit.rs:48, as launch_film_photons has it
        // (the chunks share the scratch: the stream keeps them in order)
        for (uint64_t done = 0; done < u->n_paths;) {
            const uint32_t k = (uint32_t)std::min<uint64_t>(u->n_paths - done, RL_QUERY_CHUNK);
            RL_HIP(hipEventRecord(u->timed[0].start, c.stream));
            launch_adaptive_samples(c, u, scene, seed, stream, first_path_index, (uint32_t)done, u->samples, u->rays, k);
            RL_HIP(hipGetLastError());
            RL_HIP(hipEventRecord(u->timed[0].stop, c.stream));
            RL_HIP(hipEventRecord(u->timed[1].start, c.stream));
            const int r = launch_paths(c, scene, primitive_fetch, job, first_path_index + done, u->rays, u->results, k);
            if (r != RL_OK) return r;
            RL_HIP(hipEventRecord(u->timed[1].stop, c.stream));
            g_adaptive_launches[1].fetch_add(1, std::memory_order_relaxed);
            const int r2 = timed_launch(u->timed[2], c.stream, &g_adaptive_launches[2], [&] {
                hipLaunchKernelGGL(rl_adaptive_splat_kernel, dim3(grid_for(k, c.cus)), dim3(RL_BLOCK), 0, c.stream, (const RlCameraSample*)u->samples,
                                   (const RlPathResult*)u->results, (uint64_t)k, (const RlF4*)plot->cie, plot->width, plot->height, aspect, plot->xyz);
            });
            if (r2 != RL_OK) return r2;
            done += k;
        }
        return RL_OK;
    });
    if (rc == RL_OK) u->timed_done = true;
    return rc;
}

// ---- GatherUnit-time exchange across GPUs (gather_unit.rs:49-64 with the plot buffers of G GPUs) ----

namespace {

// RCCL is bound with dlopen at the first rl_comm_* call, not at link time: the library then loads on hosts
// without RCCL (single-GPU use), and inside a process that already holds an RCCL (PyTorch ships its own copy
// under the same SONAME) the one copy in the process is shared instead of a second one being mapped.
struct RcclApi {
    void* handle = nullptr;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclCommInitAll) CommInitAll = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclReduce) Reduce = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    decltype(&ncclGetVersion) GetVersion = nullptr; // optional
    decltype(&ncclCommCount) CommCount = nullptr;   // optional: what the communicator itself says its size is
    std::string error, path;
};

RcclApi* rccl_api() {
    static RcclApi api;
    static std::once_flag once;
    std::call_once(once, [] {
        // The RCCL that belongs to the HIP runtime THIS library is running on: the one installed beside the
        // libamdhip64 that hipGetDeviceCount resolves to.  A process may hold two ROCm stacks (PyTorch bundles its own HIP,
        // HSA and RCCL under the same SONAMEs); picking RCCL by bare name can pair it with a second, uninitialised
        // HSA runtime ("no ROCm-capable device is detected").  Bare names are the fall-back.
        std::vector<std::string> names;
        Dl_info info;
        if (dladdr((void*)&hipGetDeviceCount, &info) && info.dli_fname) {
            std::string dir(info.dli_fname);
            const size_t slash = dir.rfind('/');
            if (slash != std::string::npos) {
                dir.resize(slash + 1);
                names.push_back(dir + "librccl.so.1");
                names.push_back(dir + "librccl.so");
            }
        }
        names.push_back("librccl.so.1");
        names.push_back("librccl.so");
        names.push_back("/opt/rocm/lib/librccl.so.1");
        for (const std::string& n : names) {
            api.handle = dlopen(n.c_str(), RTLD_NOW | RTLD_LOCAL);
            if (api.handle) {
                api.path = n;
                break;
            }
        }
        if (!api.handle) {
            api.error = std::string("RCCL (librccl.so.1) could not be loaded: ") + dlerror();
            return;
        }
#define RL_BIND(NAME)                                                                  \
    api.NAME = (decltype(api.NAME))dlsym(api.handle, "nccl" #NAME);                     \
    if (!api.NAME && api.error.empty()) api.error = "RCCL symbol nccl" #NAME " missing";
        RL_BIND(GetUniqueId) RL_BIND(CommInitRank) RL_BIND(CommInitAll) RL_BIND(CommDestroy) RL_BIND(Reduce)
        RL_BIND(GroupStart) RL_BIND(GroupEnd) RL_BIND(GetErrorString)
#undef RL_BIND
        api.GetVersion = (decltype(api.GetVersion))dlsym(api.handle, "ncclGetVersion");
        api.CommCount = (decltype(api.CommCount))dlsym(api.handle, "ncclCommCount");
    });
    return &api;
}

#define RL_NCCL(api, call)                                                                                  \
    do {                                                                                                    \
        ncclResult_t r_ = (call);                                                                           \
        if (r_ != ncclSuccess) return fail(RL_E_HIP, std::string(#call) + ": " + (api)->GetErrorString(r_)); \
    } while (0)

__global__ __launch_bounds__(RL_BLOCK) void rl_add_kernel(float* __restrict__ dst, const float* __restrict__ src, uint64_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * RL_BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * RL_BLOCK) dst[i] = dst[i] + src[i];
}

} // namespace

int rl_comm_unique_id(uint8_t id[RL_COMM_ID_BYTES]) {
    if (!id) return fail(RL_E_INVALID, "null id");
    RcclApi* api = rccl_api();
    if (!api->error.empty()) return fail(RL_E_NO_DEVICE, api->error);
    static_assert(sizeof(ncclUniqueId) == RL_COMM_ID_BYTES, "ncclUniqueId is 128 bytes");
    ncclUniqueId u;
    RL_NCCL(api, api->GetUniqueId(&u));
    std::memcpy(id, &u, sizeof u);
    return RL_OK;
}

int rl_comm_init_rank(const uint8_t id[RL_COMM_ID_BYTES], int world, int rank, int device, RlComm** out) {
    if (!out) return fail(RL_E_INVALID, "null output handle");
    *out = nullptr;
    if (!id || world < 1 || rank < 0 || rank >= world) return fail(RL_E_INVALID, "bad communicator arguments");
    RcclApi* api = rccl_api();
    if (!api->error.empty()) return fail(RL_E_NO_DEVICE, api->error);
    int rc = use_device(device);
    if (rc != RL_OK) return rc;
    ncclUniqueId u;
    std::memcpy(&u, id, sizeof u);
    ncclComm_t c = nullptr;
    RL_NCCL(api, api->CommInitRank(&c, world, u, rank));
    RlComm* r = new (std::nothrow) RlComm();
    if (!r) return fail(RL_E_INVALID, "out of host memory");
    r->device = device;
    r->rank = rank;
    r->world = world;
    r->nccl = c;
    *out = r;
    return RL_OK;
}

int rl_comm_init_all(const int* devices, int n, RlComm** out) {
    if (!devices || !out || n < 1) return fail(RL_E_INVALID, "bad communicator arguments");
    for (int i = 0; i < n; ++i) out[i] = nullptr;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < i; ++j)
            if (devices[i] == devices[j]) return fail(RL_E_INVALID, "an RCCL communicator needs distinct devices (one rank per GPU)");
    RcclApi* api = rccl_api();
    if (!api->error.empty()) return fail(RL_E_NO_DEVICE, api->error);
    int rc = use_device(devices[0]);
    if (rc != RL_OK) return rc;
    std::vector<ncclComm_t> comms(n, nullptr);
    RL_NCCL(api, api->CommInitAll(comms.data(), n, devices));
    for (int i = 0; i < n; ++i) {
        RlComm* r = new (std::nothrow) RlComm();
        if (!r) return fail(RL_E_INVALID, "out of host memory");
        r->device = devices[i];
        r->rank = i;
        r->world = n;
        r->nccl = comms[i];
        out[i] = r;
    }
    return RL_OK;
}

int rl_comm_destroy(RlComm* c) {
    if (!c) return RL_OK;
    RcclApi* api = rccl_api();
    (void)hipSetDevice(c->device);
    if (api->CommDestroy && c->nccl) (void)api->CommDestroy((ncclComm_t)c->nccl);
    delete c;
    return RL_OK;
}

int rl_comm_rank(const RlComm* c, int* rank, int* world) {
    if (!c) return fail(RL_E_INVALID, "null communicator");
    if (rank) *rank = c->rank;
    if (world) *world = c->world;
    return RL_OK;
}

int rl_comm_group_start(void) {
    RcclApi* api = rccl_api();
    if (!api->error.empty()) return fail(RL_E_NO_DEVICE, api->error);
    RL_NCCL(api, api->GroupStart());
    return RL_OK;
}

int rl_comm_group_end(void) {
    RcclApi* api = rccl_api();
    if (!api->error.empty()) return fail(RL_E_NO_DEVICE, api->error);
    RL_NCCL(api, api->GroupEnd());
    return RL_OK;
}

namespace {
// Reads the `n` oldest exchange timings of `u` into its totals (waits for them) and returns their events to the pool.
int exchanges_harvest(RlPlotUnit* u, size_t n) { return u->exchanges.harvest(n, &u->exchange_ms, &u->exchange_count); }
} // namespace

int rl_plot_unit_reduce(RlPlotUnit* u, RlComm* comm, int root) {
    if (!u || !comm) return fail(RL_E_INVALID, "null handle");
    if (comm->device != u->device) return fail(RL_E_STATE, "communicator rank and plot unit live on different devices");
    if (root < 0 || root >= comm->world) return fail(RL_E_INVALID, "root out of range");
    RcclApi* api = rccl_api();
    if (!api->error.empty()) return fail(RL_E_NO_DEVICE, api->error);
    int rc = use_device(u->device);
    if (rc != RL_OK) return rc;
    if ((rc = plot_settle(u)) != RL_OK) return rc; // a fused render begun into this buffer ends first
    const size_t count = (size_t)u->width * u->height * 3;
    // In place on the root; on the plot unit's stream, i.e. after every plot / fused splat into this buffer.
    // bracketed by events for rl_plot_unit_exchange_stats; a long run never asks, so the pairs are recycled and at most
    // 32 stay unread (the oldest is complete long before: it is on this unit's stream, 32 exchanges back)
    if (u->exchanges.pending.size() >= 32 && (rc = exchanges_harvest(u, 16)) != RL_OK) return rc;
    EventPair ep;
    if ((rc = u->exchanges.take(&u->ledger, &ep)) != RL_OK) return rc;
    // (Inside rl_comm_group_start / _end -- one thread driving several ranks -- RCCL enqueues the collective at GroupEnd, so both
    // events land in front of it and the exchange reads as ~0 ms: rl_plot_unit_exchange_stats is meaningful for ungrouped
    // reduces only, which is what bench.py's one-rank-per-process runs issue.)
    hipError_t he = hipEventRecord(ep.start, u->stream);
    ncclResult_t ne = ncclSuccess;
    if (he == hipSuccess) ne = api->Reduce(u->xyz, u->xyz, count, ncclFloat32, ncclSum, root, (ncclComm_t)comm->nccl, u->stream);
    if (he == hipSuccess && ne == ncclSuccess) he = hipEventRecord(ep.stop, u->stream);
    if (he != hipSuccess || ne != ncclSuccess) {
        u->exchanges.give_back(ep); // not leaked
        if (ne != ncclSuccess) return fail(RL_E_HIP, std::string("ncclReduce: ") + api->GetErrorString(ne));
        return fail(RL_E_HIP, std::string("hipEventRecord: ") + hipGetErrorString(he));
    }
    u->exchanges.pending.push_back(ep);
    return RL_OK;
}

int rl_plot_unit_exchange_stats(RlPlotUnit* u, uint64_t* exchanges, double* device_ms) {
    if (!u) return fail(RL_E_INVALID, "null plot unit");
    int rc = use_device(u->device);
    if (rc != RL_OK) return rc;
    if ((rc = exchanges_harvest(u, u->exchanges.pending.size())) != RL_OK) return rc;
    if (exchanges) *exchanges = u->exchange_count;
    if (device_ms) *device_ms = u->exchange_ms;
    return RL_OK;
}

int rl_comm_info(const RlComm* c, int* rank, int* world, int* rccl_version, char* library_path, uint32_t path_cap) {
    if (!c) return fail(RL_E_INVALID, "null communicator");
    RcclApi* api = rccl_api();
    if (!api->error.empty()) return fail(RL_E_NO_DEVICE, api->error);
    if (rank) *rank = c->rank;
    if (world) { // the communicator's own count where RCCL exports it: "did RCCL see N ranks" answered by RCCL
        int n = c->world;
        if (api->CommCount) RL_NCCL(api, api->CommCount((ncclComm_t)c->nccl, &n));
        *world = n;
    }
    if (rccl_version) {
        int v = 0;
        if (api->GetVersion) RL_NCCL(api, api->GetVersion(&v));
        *rccl_version = v;
    }
    if (library_path && path_cap) {
        std::snprintf(library_path, path_cap, "%s", api->path.c_str());
    }
    return RL_OK;
}

int rl_plot_unit_add(RlPlotUnit* dst, RlPlotUnit* src) {
    if (!dst || !src) return fail(RL_E_INVALID, "null handle");
    if (dst == src) return fail(RL_E_INVALID, "a plot unit cannot be added to itself");
    if (dst->device != src->device || dst->width != src->width || dst->height != src->height)
        return fail(RL_E_STATE, "plot units do not match (device or size)");
    int cus = 256;
    int rc = enter_device(dst->device, &cus);
    if (rc != RL_OK) return rc;
    if ((rc = plot_settle(dst)) != RL_OK || (rc = plot_settle(src)) != RL_OK) return rc; // begun fused renders end first
    const uint64_t n = (uint64_t)dst->width * dst->height * 3;
    if ((rc = hand_over(src->ready, src->stream, dst->stream)) != RL_OK) return rc; // everything written into src so far is added
    hipLaunchKernelGGL(rl_add_kernel, dim3(grid_for(n, cus)), dim3(RL_BLOCK), 0, dst->stream, dst->xyz, src->xyz, n);
    RL_HIP(hipGetLastError());
    return hand_over(dst->plotted, dst->stream, src->stream); // src may be cleared or splatted into only after it was read
}

int rl_gather_unit_allreduce(RlGatherUnit* gather, RlPlotUnit* plot, RlComm* comm) {
    if (!plot || !comm) return fail(RL_E_INVALID, "null handle");
    if (comm->rank == 0 && !gather) return fail(RL_E_INVALID, "rank 0 accumulates: it needs the gather unit");
    int rc = rl_plot_unit_reduce(plot, comm, 0);
    if (rc != RL_OK) return rc;
    if (comm->rank == 0) return rl_gather_unit_accumulate(gather, plot); // Kahan + clear (gather_unit.rs:49-64, app.rs:147)
    return rl_plot_unit_clear(plot);
}

// Diagnostics: how many launches carried k blocking render calls (k = 1 .. 256) on `device` since the library was
// loaded; out holds 257 counters.
int rl_debug_batch_histogram(int device, uint64_t* out) {
    if (!out) return fail(RL_E_INVALID, "null argument");
    for (uint32_t k = 0; k <= RL_OPEN_CAP; ++k) out[k] = 0;
    int rc = use_device(device);
    if (rc == RL_OK) rc = sessions_quiesce(device); // the open launches still running end first: then they are counted
    if (rc != RL_OK) return rc;
    DeviceSessions* d = sessions_of(device);
    std::lock_guard<std::mutex> guard(d->lock);
    for (uint32_t k = 0; k <= RL_OPEN_CAP; ++k) out[k] += d->histogram[k];
    if (getenv("RL_OPEN_LAUNCH_TIMING") && d->calls)
        fprintf(stderr, "open launches on device %d: %llu calls, mean us per call: wait for the target %.1f, admission %.1f, completion %.1f\n",
                device, (unsigned long long)d->calls, d->presync_us / d->calls, d->admit_us / d->calls, d->wait_us / d->calls);
    d->presync_us = d->admit_us = d->wait_us = 0.0;
    d->calls = 0;
    return RL_OK;
}

// Diagnostics: launches of each of the 24 instantiations of the trace kernel since the library was loaded; index = 8 * (the whole
// scene staged in LDS) + 4 * (fused with the splat) + 2 * (open launch) + 1 * (prisms with a second bound), and 16 + the low three
// bits for the instantiations that stage the tables only (trace_kernel_variant).
int rl_debug_variant_launches(uint64_t* out) {
    if (!out) return fail(RL_E_INVALID, "null argument");
    for (int k = 0; k < 24; ++k) out[k] = g_variant_launches[k].load(std::memory_order_relaxed);
    return RL_OK;
}

int rl_debug_wavelength_variant_launches(uint64_t out[24]) {
    if (!out) return fail(RL_E_INVALID, "null argument");
    for (int k = 0; k < 24; ++k) out[k] = g_wavelength_variant_launches[k].load(std::memory_order_relaxed);
    return RL_OK;
}

int rl_debug_query_launches(uint64_t* out) { return family_launches(g_query_kernels, out); }
int rl_debug_occlusion_launches(uint64_t* out) { return family_launches(g_occlusion_kernels, out); }
int rl_debug_path_launches(uint64_t* out) { return family_launches(g_path_kernels, out); }
int rl_debug_film_launches(uint64_t* out) { return family_launches(g_film_kernels, out); }
int rl_debug_step_launches(uint64_t* out) { return family_launches(g_step_kernels, out); }
int rl_debug_path_list_launches(uint64_t* out) { return family_launches(g_list_step_kernels, out); }
int rl_debug_light_launches(uint64_t* out) { return family_launches(g_light_kernels, out); }
int rl_debug_light_film_launches(uint64_t* out) { return family_launches(g_light_film_kernels, out); }
int rl_debug_direct_launches(uint64_t out[6]) { return family_launches(g_direct_kernels, out); }
int rl_debug_feature_launches(uint64_t out[6]) { return family_launches(g_feature_kernels, out); }

int rl_debug_denoise_launches(uint64_t out[2]) {
    if (!out) return fail(RL_E_INVALID, "null output");
    for (int k = 0; k < 2; ++k) out[k] = g_denoise_launches[k].load(std::memory_order_relaxed);
    return RL_OK;
}
int rl_debug_denoise_variance_launches(uint64_t out[2]) {
    if (!out) return fail(RL_E_INVALID, "null output");
    for (int k = 0; k < 2; ++k) out[k] = g_denoise_variance_launches[k].load(std::memory_order_relaxed);
    return RL_OK;
}
int rl_debug_denoise_variance_ms(RlDenoiseUnit* u, float* ms) {
    if (!u || !ms) return fail(RL_E_INVALID, "null argument");
    int rc = use_device(u->device);
    if (rc != RL_OK) return rc;
    *ms = 0.0f;
    if (u->timed_variance_done) RL_HIP(hipEventElapsedTime(ms, u->timed_variance.start, u->timed_variance.stop));
    return RL_OK;
}
int rl_debug_spectral_launches(uint64_t out[2]) {
    if (!out) return fail(RL_E_INVALID, "null output");
    for (int k = 0; k < 2; ++k) out[k] = g_spectral_launches[k].load(std::memory_order_relaxed);
    return RL_OK;
}
int rl_debug_spectral_ms(RlSpectralUnit* u, float out[2]) {
    if (!u || !out) return fail(RL_E_INVALID, "null argument");
    int rc = use_device(u->device);
    if (rc != RL_OK) return rc;
    for (int k = 0; k < 2; ++k) {
        out[k] = 0.0f;
        if (u->timed_done[k]) RL_HIP(hipEventElapsedTime(&out[k], u->timed[k].start, u->timed[k].stop));
    }
    return RL_OK;
}
int rl_debug_glare_launches(uint64_t* out) {
    if (!out) return fail(RL_E_INVALID, "null output");
    *out = g_glare_launches.load(std::memory_order_relaxed);
    return RL_OK;
}
int rl_debug_glare_ms(RlGlareUnit* u, float* ms) {
    if (!u || !ms) return fail(RL_E_INVALID, "null argument");
    int rc = use_device(u->device);
    if (rc != RL_OK) return rc;
    *ms = 0.0f;
    if (u->timed_done) RL_HIP(hipEventElapsedTime(ms, u->timed.start, u->timed.stop));
    return RL_OK;
}
int rl_debug_relight_launches(uint64_t out[3]) {
    if (!out) return fail(RL_E_INVALID, "null output");
    for (int k = 0; k < 3; ++k) out[k] = g_relight_launches[k].load(std::memory_order_relaxed);
    return RL_OK;
}
int rl_debug_relight_ms(RlRelightUnit* u, float out[3]) {
    if (!u || !out) return fail(RL_E_INVALID, "null argument");
    int rc = use_device(u->device);
    if (rc != RL_OK) return rc;
    for (int k = 0; k < 3; ++k) {
        out[k] = 0.0f;
        if (u->timed_done[k]) RL_HIP(hipEventElapsedTime(&out[k], u->timed[k].start, u->timed[k].stop));
    }
    return RL_OK;
}
int rl_debug_error_launches(uint64_t out[2]) {
    if (!out) return fail(RL_E_INVALID, "null output");
    for (int k = 0; k < 2; ++k) out[k] = g_error_launches[k].load(std::memory_order_relaxed);
    return RL_OK;
}
int rl_debug_error_ms(RlErrorUnit* u, float out[2]) {
    if (!u || !out) return fail(RL_E_INVALID, "null argument");
    int rc = use_device(u->device);
    if (rc != RL_OK) return rc;
    for (int k = 0; k < 2; ++k) {
        out[k] = 0.0f;
        if (!u->timed_done[k]) continue;
        RL_HIP(hipEventSynchronize(u->timed[k].stop));
        RL_HIP(hipEventElapsedTime(&out[k], u->timed[k].start, u->timed[k].stop));
    }
    return RL_OK;
}
int rl_debug_robust_launches(uint64_t out[2]) {
    if (!out) return fail(RL_E_INVALID, "null output");
    for (int k = 0; k < 2; ++k) out[k] = g_robust_launches[k].load(std::memory_order_relaxed);
    return RL_OK;
}
int rl_debug_robust_ms(RlRobustUnit* u, float out[2]) {
    if (!u || !out) return fail(RL_E_INVALID, "null argument");
    int rc = use_device(u->device);
    if (rc != RL_OK) return rc;
    for (int k = 0; k < 2; ++k) {
        out[k] = 0.0f;
        if (!u->timed_done[k]) continue;
        RL_HIP(hipEventSynchronize(u->timed[k].stop));
        RL_HIP(hipEventElapsedTime(&out[k], u->timed[k].start, u->timed[k].stop));
    }
    return RL_OK;
}
int rl_debug_robust_estimate_launches(uint64_t* out) {
    if (!out) return fail(RL_E_INVALID, "null output");
    *out = g_robust_estimate_launches.load(std::memory_order_relaxed);
    return RL_OK;
}
int rl_debug_robust_estimate_ms(RlRobustUnit* u, float* out) {
    if (!u || !out) return fail(RL_E_INVALID, "null argument");
    int rc = use_device(u->device);
    if (rc != RL_OK) return rc;
    *out = 0.0f;
    if (!u->timed_estimate_done) return RL_OK;
    RL_HIP(hipEventSynchronize(u->timed_estimate.stop));
    RL_HIP(hipEventElapsedTime(out, u->timed_estimate.start, u->timed_estimate.stop));
    return RL_OK;
}
int rl_debug_adaptive_launches(uint64_t out[3]) {
    if (!out) return fail(RL_E_INVALID, "null output");
    for (int k = 0; k < 3; ++k) out[k] = g_adaptive_launches[k].load(std::memory_order_relaxed);
    return RL_OK;
}
int rl_debug_adaptive_ms(RlAdaptiveUnit* u, float out[3]) {
    if (!u || !out) return fail(RL_E_INVALID, "null argument");
    int rc = use_device(u->device);
    if (rc != RL_OK) return rc;
    for (int k = 0; k < 3; ++k) {
        out[k] = 0.0f;
        if (!u->timed_done) continue;
        RL_HIP(hipEventSynchronize(u->timed[k].stop));
        RL_HIP(hipEventElapsedTime(&out[k], u->timed[k].start, u->timed[k].stop));
    }
    return RL_OK;
}
int rl_debug_gather_accumulate_ms(RlGatherUnit* u, RlPlotUnit* plot, float* ms) {
    if (!u || !plot || !ms) return fail(RL_E_INVALID, "null argument");
    int rc = use_device(u->device);
    if (rc != RL_OK) return rc;
    if ((rc = plot_settle(plot)) != RL_OK) return rc;
    if (plot->device == u->device) RL_HIP(hipStreamSynchronize(plot->stream));
    RL_HIP(hipStreamSynchronize(u->stream));
    EventPair ep;
    if ((rc = u->timed.take(&u->ledger, &ep)) != RL_OK) return rc;
    hipError_t e = hipEventRecord(ep.start, u->stream);
    if (e == hipSuccess) rc = rl_gather_unit_accumulate(u, plot);
    if (e == hipSuccess && rc == RL_OK) e = hipEventRecord(ep.stop, u->stream);
    if (e != hipSuccess || rc != RL_OK) {
        u->timed.give_back(ep);
        if (rc != RL_OK) return rc;
        RL_HIP(e);
    }
    u->timed.pending.push_back(ep);
    double total = 0.0;
    uint64_t read = 0;
    rc = u->timed.harvest(1, &total, &read); // waits for the launch
    *ms = (float)total;
    return rc;
}

int rl_debug_live_resources(uint64_t out[4]) {
    if (!out) return fail(RL_E_INVALID, "null output");
    for (int k = 0; k < LIVE_KINDS; ++k) out[k] = g_live[k].load(std::memory_order_relaxed);
    return RL_OK;
}
int rl_debug_denoise_pass_ms(RlDenoiseUnit* u, float out[1 + RL_DENOISE_MAX_ITERATIONS]) {
    if (!u || !out) return fail(RL_E_INVALID, "null argument");
    int rc = use_device(u->device);
    if (rc != RL_OK) return rc;
    for (uint32_t k = 0; k <= RL_DENOISE_MAX_ITERATIONS; ++k) {
        out[k] = 0.0f;
        if (u->timed_passes != 0u && k <= u->timed_passes) RL_HIP(hipEventElapsedTime(&out[k], u->timed[k].start, u->timed[k].stop));
    }
    return RL_OK;
}

int rl_debug_scene_emitters(const RlObjectDesc* objects, uint32_t n_objects, uint32_t* out, uint32_t cap, uint32_t* n_emitters) {
    if ((!objects && n_objects) || !n_emitters) return fail(RL_E_INVALID, "null argument");
    std::vector<RlF4> table;
    std::vector<uint32_t> indices;
    emitter_table(objects, n_objects, &table, &indices);
    *n_emitters = (uint32_t)indices.size();
    if (indices.empty()) return RL_OK;
    if (!out || cap < indices.size()) return fail(RL_E_INVALID, "index array too small for the description's emitters");
    std::memcpy(out, indices.data(), indices.size() * sizeof(uint32_t));
    return RL_OK;
}

int rl_debug_light_sample(const RlObjectDesc* objects, uint32_t n_objects, uint64_t seed, uint32_t stream, const RlPathState* states,
                          const RlRayHit* hits, uint32_t n, RlLightSample* samples, RlRay* rays) {
    if ((!objects && n_objects) || (n && (!states || !hits || !samples))) return fail(RL_E_INVALID, "null argument");
    std::vector<RlF4> table, records(n_objects);
    std::vector<uint32_t> indices;
    emitter_table(objects, n_objects, &table, &indices);
    for (uint32_t i = 0; i < n_objects; ++i) // (the object records as far as rl_light_sample reads them: the material kind)
        records[i] = RlF4{objects[i].m0, objects[i].m1, objects[i].m2, rl_u2f(rl_object_bits(objects[i].surface_kind, objects[i].material_kind, 0u))};
    for (uint32_t i = 0; i < n; ++i) {
        const RlPathState& st = states[i];
        const RlRayHit& h = hits[i];
        const RlLightDraw s = rl_light_sample(records.data(), n_objects, table.data(), (uint32_t)indices.size(), seed, stream, st.path_index, st.segments, st.end,
                                              st.wavelength, rl_f3(st.direction.x, st.direction.y, st.direction.z),
                                              rl_f3(h.isect.position.x, h.isect.position.y, h.isect.position.z),
                                              rl_f3(h.isect.normal.x, h.isect.normal.y, h.isect.normal.z), h.object);
        const bool cast = s.status == RL_LIGHT_VISIBLE;
        RlLightSample out;
        out.direction = RlVector3{s.direction.x, s.direction.y, s.direction.z};
        out.distance = s.distance;
        out.value = cast ? st.intensity * s.weight : 0.0f;
        out.weight = s.weight;
        out.emitter = s.emitter;
        out.status = s.status;
        samples[i] = out;
        if (rays) {
            RlRay r;
            std::memset(&r, 0, sizeof r);
            if (cast) {
                r.origin = RlVector3{s.origin.x, s.origin.y, s.origin.z};
                r.direction = out.direction;
                r.t_max = s.t_max;
            }
            rays[i] = r;
        }
    }
    return RL_OK;
}

// ---- device-side math probe (tests) -------------------------------------------------------------

// Not part of the reference's interface: evaluates csrc/rl_math.h on the GPU so the tests can
// verify that hipcc and g++ agree bit-for-bit.  fn as in rl_math_probe_kernel.
int rl_debug_math_probe(int device, int fn, const float* x, float* y, uint32_t n) {
    if (!x || !y || n == 0) return fail(RL_E_INVALID, "null argument");
    int rc = use_device(device);
    if (rc != RL_OK) return rc;
    float *dx = nullptr, *dy = nullptr;
    RL_HIP(hipMalloc((void**)&dx, n * sizeof(float)));
    hipError_t e = hipMalloc((void**)&dy, n * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(dx, x, n * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(rl_math_probe_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, fn, dx, dy, n);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(y, dy, n * sizeof(float), hipMemcpyDeviceToHost);
    (void)hipFree(dx);
    if (dy) (void)hipFree(dy);
    if (e != hipSuccess) return fail(RL_E_HIP, std::string("math probe: ") + hipGetErrorString(e));
    return RL_OK;
}

// The short forms (fn 16 rl_sqrtf, 17 rl_recipf, 18 rl_div200f) against the compiler's IEEE expansions for every float with bits in
// [lo_bits, hi_bits) -- and its negative when both_signs -- on the device.  counts[0] = arguments that differ, counts[1] = arguments
// compared; *example = one argument that differs (bits), if any.
int rl_debug_math_sweep(int device, int fn, uint32_t lo_bits, uint32_t hi_bits, int both_signs, uint64_t* counts, uint32_t* example) {
    if (!counts || !example || fn < 16 || fn > 18 || hi_bits <= lo_bits) return fail(RL_E_INVALID, "math sweep: fn 16..18, lo < hi");
    int rc = use_device(device);
    if (rc != RL_OK) return rc;
    unsigned long long* bad = nullptr;
    RL_HIP(hipMalloc((void**)&bad, 32));
    hipError_t e = hipMemset(bad, 0, 32);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(rl_math_sweep_kernel, dim3(8192), dim3(RL_BLOCK), 0, 0, fn, lo_bits, hi_bits, both_signs, bad, (uint32_t*)(bad + 2));
        e = hipGetLastError();
    }
    unsigned long long host[4] = {0, 0, 0, 0};
    if (e == hipSuccess) e = hipMemcpy(host, bad, 32, hipMemcpyDeviceToHost);
    (void)hipFree(bad);
    if (e != hipSuccess) return fail(RL_E_HIP, std::string("math sweep: ") + hipGetErrorString(e));
    counts[0] = host[0];
    counts[1] = host[1];
    *example = (uint32_t)host[2];
    return RL_OK;
}

int rl_debug_prism_count(const RlScene* scene, uint32_t* n_prisms) {
    if (!scene || !n_prisms) return fail(RL_E_INVALID, "null argument");
    *n_prisms = scene->lay.n_prisms;
    return RL_OK;
}

int rl_debug_prism_probe(const RlScene* scene, uint32_t prism, const float* rays, uint32_t n, uint32_t* out) {
    if (!scene || !rays || !out) return fail(RL_E_INVALID, "null argument");
    if (prism >= scene->lay.n_prisms) return fail(RL_E_INVALID, "no such prism");
    if (n == 0) return RL_OK;
    int rc = use_device(scene->device);
    if (rc != RL_OK) return rc;
    float* dr = nullptr;
    uint32_t* dout = nullptr;
    hipError_t e = hipMalloc((void**)&dr, (size_t)n * 6 * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&dout, (size_t)n * 5 * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemcpy(dr, rays, (size_t)n * 6 * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(rl_prism_probe_kernel, dim3((n + 255) / 256), dim3(256), 0, 0,
                           scene->blob + scene->lay.off_prisms + (size_t)RL_PRISM_STRIDE * prism, dr, n, dout);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(out, dout, (size_t)n * 5 * sizeof(uint32_t), hipMemcpyDeviceToHost);
    if (dr) (void)hipFree(dr);
    if (dout) (void)hipFree(dout);
    if (e != hipSuccess) return fail(RL_E_HIP, std::string("prism probe: ") + hipGetErrorString(e));
    return RL_OK;
}

#ifdef RL_STATS
// Diagnostic build only (not in the header): copies and clears the trace kernel's event counters.
int rl_stats_read(unsigned long long* out, int n) {
    unsigned long long host[48];
    if (hipDeviceSynchronize() != hipSuccess) return RL_E_HIP;
    if (hipMemcpyFromSymbol(host, HIP_SYMBOL(rl_stat_counters), sizeof host) != hipSuccess) return RL_E_HIP;
    for (int i = 0; i < n && i < 48; ++i) out[i] = host[i];
    std::memset(host, 0, sizeof host);
    if (hipMemcpyToSymbol(HIP_SYMBOL(rl_stat_counters), host, sizeof host) != hipSuccess) return RL_E_HIP;
    return RL_OK;
}
#endif

} // extern "C"
