// capi.hip — the C ABI of include/vqhip.h: argument validation, the per-call constant ring (the
// analogue of the reference's DynamicBufferHeap upload heap) and kernel dispatch. There is no CPU
// fallback anywhere in this library: without a gfx950 device vqhip_create() fails and every other
// entry point needs a context.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <dlfcn.h>
#include <algorithm>
#include <atomic>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>
#include "vq_internal.h"
#include "vq_devmath.h"      // vqd::sincos_ is __host__ __device__: frame-uniform trigonometry is evaluated here, once

using namespace vqk;

struct vqhip_ctx {
    int device = 0;
    int nCUs = 256;
    int ldsPerBlock = 64 * 1024;   // hipDeviceAttributeMaxSharedMemoryPerBlock (163 840 on gfx950): what a kernel may opt into, queried once in vqhip_create
    static constexpr int kSlots = 32;
    char* hostRing = nullptr;      // pinned
    char* devRing = nullptr;
    hipEvent_t slotEvent[kSlots] = {};
    hipStream_t copyStream = nullptr;          // constants are uploaded on their own stream: the DMA of call n+1 overlaps the kernels of call n
    hipEvent_t copyEvent[kSlots] = {};
    bool slotBusy[kSlots] = {};
    int nextSlot = 0;
    void* scratch = nullptr; size_t scratchBytes = 0;
    // footprint records of the diffuse convolution (conv.hip:k_diffuse_records): rewritten by every vqhip_conv_diffuse; `recFree` is recorded behind the
    // kernel that reads them, and the next call's stream waits for it before it overwrites them (calls may come on different streams)
    void* rec = nullptr; size_t recBytes = 0; hipEvent_t recFree = nullptr; bool recUsed = false;
    // edge-pixel list of vqhip_forward_lighting_msaa (msaa.hip): a counter + 4 B per pixel. Its own buffer, not `scratch` (the post chain's two-kernel form keeps
    // BlurIntermediate there, possibly on another stream next to shading); `edgeFree` is recorded behind the kernel that reads it, the next call's stream waits for it
    void* edge = nullptr; size_t edgeBytes = 0; hipEvent_t edgeFree = nullptr; bool edgeUsed = false;
    // per-tile minima of the depth hierarchy's TRUE_TOP form (depth.hip: k_depth_hierarchy writes them, k_depth_tail reduces them): kMaxDepthTiles floats, allocated
    // on first use; `hierFree` orders calls on different streams, as `edgeFree` does for the edge list
    void* hier = nullptr; hipEvent_t hierFree = nullptr; bool hierUsed = false;
    // per-tile ray counts and tile flags of vqhip_ssr_classify (ssr_trace.hip: count -> scan -> scatter): 2 x kMaxSsrTiles dwords, allocated on first use;
    // `ssrFree` orders calls on different streams, as `hierFree` does
    void* ssrTiles = nullptr; hipEvent_t ssrFree = nullptr; bool ssrUsed = false;
    int pow5ExpLog = 0;            // vqhip_set_fresnel_pow
    int arithDxc = 0;              // vqhip_set_arithmetic
    vqk::Options opt;              // vqhip_set_option
    // 65536-entry tonemap tables (post.hip:k_tonemap_lut), cached per (TonemapperParams, output format): the table is built once
    // per parameter set instead of once per frame. Streams that HIT a cached table only wait for the event of its build. A table is replaced
    // only when a fifth parameter set shows up: the least recently used one goes (a hit counts as a use). Every use records the slot's `lastUse` event
    // behind the kernel that read the table; the rebuild makes ITS stream wait for that event — no host stall, legal under stream capture. Only a table
    // that has been read from MORE THAN ONE stream (one event cannot cover readers on several streams) is replaced after a device-wide wait.
    static constexpr int kLuts = 4;
    struct TonemapLut { void* table = nullptr; VQ_TonemapperParams key{}; int outFmt = -1; bool valid = false;
                        hipEvent_t built = nullptr, lastUse = nullptr; hipStream_t lastStream = nullptr; bool used = false, multiStream = false, everBuilt = false;
                        uint64_t lastUseTick = 0; } lut[kLuts];
    uint64_t lutTick = 0;
    // one thread at a time per context: entry points detect a second thread inside the same context and refuse it
    std::atomic<uint64_t> owner{0};            // token of the thread inside an entry point (0: nobody); acquired by CAS, cleared by the outermost guard
    int ownerDepth = 0;                        // nesting depth: touched by the owner only
    uint64_t generation = 0;                   // distinguishes this context from an earlier one at the same address (vqhip_last_error)
    std::string lastError;
};

namespace {

thread_local std::string g_lastError;
thread_local const vqhip_ctx* g_lastErrorCtx = nullptr;     // the context this thread's most recent failure belongs to (vqhip_last_error) ...
thread_local uint64_t g_lastErrorGen = 0;                   // ... and its generation: a later context at the same address does not inherit the message
std::atomic<uint64_t> g_ctxGeneration{1};

int fail(vqhip_ctx* ctx, int code, const std::string& msg) {
    g_lastError = msg;
    g_lastErrorCtx = ctx;
    g_lastErrorGen = ctx ? ctx->generation : 0;
    if (ctx) ctx->lastError = msg;
    return code;
}
// a call refused because ANOTHER thread is inside the context: the message stays with the refused thread, the context is not written to
int failRefused(const vqhip_ctx* ctx, const std::string& msg) {
    g_lastError = msg;
    g_lastErrorCtx = ctx;
    g_lastErrorGen = ctx ? ctx->generation : 0;
    return VQHIP_ERR_INVALID_ARG;
}
int failHip(vqhip_ctx* ctx, hipError_t e, const char* what) {
    return fail(ctx, VQHIP_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}
#define HIP_TRY(ctx, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return failHip(ctx, e_, #call); } while (0)

bool isImageFmt(int f) { return f == VQHIP_FMT_RGBA32F || f == VQHIP_FMT_RGBA16F; }

// Acquire the next constant-ring slot (waits for the kernel that last read it, if still in flight).
int acquireSlot(vqhip_ctx* ctx, int* slot) {
    const int s = ctx->nextSlot;
    ctx->nextSlot = (s + 1) % vqhip_ctx::kSlots;
    if (ctx->slotBusy[s]) { HIP_TRY(ctx, hipEventSynchronize(ctx->slotEvent[s])); ctx->slotBusy[s] = false; }
    *slot = s;
    return VQHIP_OK;
}
int commitSlot(vqhip_ctx* ctx, int slot, size_t bytes, hipStream_t st) {
    // The slot is free (acquireSlot waited for its last reader), so the copy need not queue behind the caller's stream: it
    // runs on the context's copy stream right away and the caller's stream only waits for its completion event.
    HIP_TRY(ctx, hipMemcpyAsync(ctx->devRing + (size_t)slot * kConstSlotBytes, ctx->hostRing + (size_t)slot * kConstSlotBytes, bytes, hipMemcpyHostToDevice, ctx->copyStream));
    HIP_TRY(ctx, hipEventRecord(ctx->copyEvent[slot], ctx->copyStream));
    HIP_TRY(ctx, hipStreamWaitEvent(st, ctx->copyEvent[slot], 0));
    return VQHIP_OK;
}
int releaseSlot(vqhip_ctx* ctx, int slot, hipStream_t st) {
    HIP_TRY(ctx, hipEventRecord(ctx->slotEvent[slot], st));
    ctx->slotBusy[slot] = true;
    return VQHIP_OK;
}
// One constant block of the lit draws into the next ring slot: acquire the slot, fill it (fillFrameConstants or fillGbufConstants with `args`), commit it in front
// of `st`. *dev = where the kernels read the block; the caller releases *slot behind the kernel that reads it
template <class Block, class Fill, class... Args>
int stageConstants(vqhip_ctx* ctx, hipStream_t st, int* slot, const Block** dev, Fill fill, Args... args) {
    if (const int rc = acquireSlot(ctx, slot)) return rc;
    const size_t bytes = fill(ctx, *slot, args...);
    *dev = (const Block*)(ctx->devRing + (size_t)*slot * kConstSlotBytes);
    return commitSlot(ctx, *slot, bytes, st);
}
// the four planes of a vqhip_gbuffer as a kernel's arguments take them (to read or to write); false: one is NULL, and the caller words the refusal
template <class Args>
bool gbufferPlanes(const vqhip_gbuffer& g, Args* a) {
    using P = decltype(a->gb0);
    a->gb0 = (P)g.gb0; a->gb1 = (P)g.gb1; a->gb2 = (P)g.gb2; a->gb3 = (P)g.gb3;
    return g.gb0 && g.gb1 && g.gb2 && g.gb3;
}

int ensureScratch(vqhip_ctx* ctx, size_t bytes) {
    if (ctx->scratchBytes >= bytes) return VQHIP_OK;
    if (ctx->scratch) { HIP_TRY(ctx, hipDeviceSynchronize()); HIP_TRY(ctx, hipFree(ctx->scratch)); ctx->scratch = nullptr; ctx->scratchBytes = 0; }
    HIP_TRY(ctx, hipMalloc(&ctx->scratch, bytes));
    ctx->scratchBytes = bytes;
    return VQHIP_OK;
}

// The tonemap table of (p, outFmt), ready to be read by work enqueued on `st` after this call: a cached table makes `st` wait for the
// event of its build (it may have happened on another stream); a miss rebuilds the LEAST RECENTLY USED slot on `st` — behind the slot's last-use
// event when all its readers were on one stream, after a device-wide wait when they were on several (releaseTonemapLut keeps the record).
int acquireTonemapLut(vqhip_ctx* ctx, hipStream_t st, const VQ_TonemapperParams& p, int outFmt, int* slotOut) {
    int victim = 0;
    for (int i = 0; i < vqhip_ctx::kLuts; ++i) {
        auto& L = ctx->lut[i];
        if (L.valid && L.outFmt == outFmt && std::memcmp(&L.key, &p, sizeof(p)) == 0) {
            HIP_TRY(ctx, hipStreamWaitEvent(st, L.built, 0));
            L.lastUseTick = ++ctx->lutTick;
            *slotOut = i;
            return VQHIP_OK;
        }
        if (!L.valid) { if (ctx->lut[victim].valid) victim = i; }
        else if (ctx->lut[victim].valid && L.lastUseTick < ctx->lut[victim].lastUseTick) victim = i;
    }
    auto& L = ctx->lut[victim];
    // Whatever state an earlier failure left the slot in (valid or not), the rebuild must queue behind every kernel that may still read the table and
    // behind the last build that wrote it: `used` / `lastUse` / `built` survive an invalidation and are only reset once the NEW build is enqueued.
    if (L.used) {
        if (L.multiStream) HIP_TRY(ctx, hipDeviceSynchronize());            // readers on several streams: one event does not cover them (documented in vqhip.h)
        else HIP_TRY(ctx, hipStreamWaitEvent(st, L.lastUse, 0));              // the rebuild queues behind the last kernel that read the table
    } else if (L.everBuilt) {
        HIP_TRY(ctx, hipStreamWaitEvent(st, L.built, 0));                     // built (possibly on another stream) and never read: write after write
    }
    L.valid = false;
    hipError_t e = launch_tonemap_lut_build(st, L.table, p, outFmt);
    if (e != hipSuccess) return failHip(ctx, e, "tonemap table build launch");
    HIP_TRY(ctx, hipEventRecord(L.built, st));
    L.key = p; L.outFmt = outFmt; L.valid = true; L.everBuilt = true; L.used = false; L.multiStream = false; L.lastStream = nullptr; L.lastUseTick = ++ctx->lutTick;
    *slotOut = victim;
    return VQHIP_OK;
}
// called behind the kernel that read table `slot` on `st`
int releaseTonemapLut(vqhip_ctx* ctx, hipStream_t st, int slot) {
    auto& L = ctx->lut[slot];
    if (L.used && L.lastStream != st) L.multiStream = true;
    HIP_TRY(ctx, hipEventRecord(L.lastUse, st));
    L.used = true; L.lastStream = st;
    return VQHIP_OK;
}

// RAII marker of "this thread is inside an entry point of ctx". A second THREAD entering the same context while one is inside is refused
// (VQHIP_ERR_INVALID_ARG) instead of corrupting the constant ring / table cache; nested calls of the same thread (vqhip_post_process ->
// vqhip_gaussian_blur_x) pass. The context may migrate between threads, it just cannot be shared at the same time.
// Ownership is ONE atomic word holding a per-thread token: a thread enters by CAS 0 -> its token, so there is no window in which another thread can
// read a stale owner; a nested call recognises its own token and bumps a depth counter only the owner touches; the outermost guard clears the word.
uint64_t threadToken() {
    static std::atomic<uint64_t> next{1};
    thread_local const uint64_t t = next.fetch_add(1, std::memory_order_relaxed);
    return t;
}
struct CtxGuard {
    vqhip_ctx* c; bool ok;
    explicit CtxGuard(vqhip_ctx* ctx) : c(ctx), ok(true) {
        if (!c) return;
        const uint64_t me = threadToken();
        if (c->owner.load(std::memory_order_acquire) == me) { ++c->ownerDepth; return; }      // nested call of the owner
        uint64_t expected = 0;
        if (!c->owner.compare_exchange_strong(expected, me, std::memory_order_acq_rel)) { ok = false; c = nullptr; return; }
        c->ownerDepth = 1;
    }
    ~CtxGuard() { if (c && --c->ownerDepth == 0) c->owner.store(0, std::memory_order_release); }
};
#define CTX_GUARD(ctx, who) CtxGuard guard_(ctx); if (!guard_.ok) return failRefused(ctx, std::string(who) + ": the context is in use on another thread (one thread at a time per vqhip_ctx)")

int mipDim(int d0, int l) { int d = d0 >> l; return d < 1 ? 1 : d; }

// Smallest float t >= 0 with sqrtf(t) >= range: `length(Lw - P) < range` (Lighting.hlsl:318) <=> `dot(d,d) < t` exactly, because the
// correctly rounded sqrt is monotonic. NaN range -> NaN (never lit); range <= 0 -> 0 (never lit); +inf -> +inf (every finite distance).
float rangeCullThreshold(float range) {
    if (!(range == range)) return range;
    if (range <= 0.0f) return 0.0f;
    if (range == INFINITY) return INFINITY;
    const double r2 = (double)range * (double)range;
    float t = r2 >= (double)FLT_MAX ? FLT_MAX : (float)r2;
    while (t > 0.0f && sqrtf(t) >= range) t = nextafterf(t, 0.0f);           // now sqrtf(t) < range (or t == 0)
    while (sqrtf(t) < range) { if (t == FLT_MAX) return INFINITY; t = nextafterf(t, INFINITY); }
    return t;
}

// The bytes from a plane's first pixel to the end of its last row: `height` rows of `width` pixels of `bpp` bytes, `pitchPx` pixels apart. Every front end measures with this
size_t planeExtent(int width, int height, size_t pitchPx, size_t bpp) { return ((size_t)(height - 1) * pitchPx + (size_t)width) * bpp; }
bool rangesOverlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a && b && a0 < b0 + nb && b0 < a0 + na;
}
struct Span { const void* p; size_t n; const char* name; };                           // the bytes that a plane, a per-tile buffer or a list covers; p NULL: nothing
// The overlap questions of the front ends: one span against a list (the quad-uv plane against a draw's outputs, an input against a pass's outputs), a list against itself
bool overlapsAny(const Span& s, const Span* outs, int nOut) {
    for (int i = 0; i < nOut; ++i) if (rangesOverlap(s.p, s.n, outs[i].p, outs[i].n)) return true;
    return false;
}
bool overlapEachOther(const Span* outs, int nOut) {
    for (int i = 0; i + 1 < nOut; ++i) if (overlapsAny(outs[i], outs + i + 1, nOut - i - 1)) return true;
    return false;
}

} // namespace

namespace vqk { int fail_global(int code, const std::string& msg) { return fail(nullptr, code, msg); } }     // for mgpu.hip (no context)

namespace vqk {
namespace {
struct Roctx { int (*push)(const char*) = nullptr; int (*pop)() = nullptr; };
const Roctx& roctx() {
    static const Roctx r = [] {
        Roctx x;
        const char* env = std::getenv("VQHIP_ROCTX");
        if (env && env[0] == '0') return x;
        for (const char* n : { "librocprofiler-sdk-roctx.so.1", "libroctx64.so.4", "libroctx64.so" }) {
            if (void* lib = dlopen(n, RTLD_NOW | RTLD_LOCAL)) {
                x.push = (int (*)(const char*))dlsym(lib, "roctxRangePushA");
                x.pop = (int (*)())dlsym(lib, "roctxRangePop");
                if (x.push && x.pop) return x;
                x = Roctx{};
            }
        }
        return x;
    }();
    return r;
}
} // namespace
Range::Range(const char* name) : on(roctx().push != nullptr) { if (on) roctx().push(name); }
Range::~Range() { if (on) roctx().pop(); }
} // namespace vqk

extern "C" {

int vqhip_abi_version(void) { return VQHIP_ABI_VERSION; }

// the calling thread's own most recent failure when it belongs to `ctx` (race-free, and the only record of a refused concurrent call), else the context's
const char* vqhip_last_error(const vqhip_ctx* ctx) { return (!ctx || (g_lastErrorCtx == ctx && g_lastErrorGen == ctx->generation)) ? g_lastError.c_str() : ctx->lastError.c_str(); }

int vqhip_create(int device_ordinal, vqhip_ctx** out_ctx) {
    if (!out_ctx) return fail(nullptr, VQHIP_ERR_INVALID_ARG, "vqhip_create: out_ctx is NULL");
    *out_ctx = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) return fail(nullptr, VQHIP_ERR_NO_DEVICE, "vqhip_create: no HIP device visible (this library has no CPU fallback)");
    if (device_ordinal < 0 || device_ordinal >= n) return fail(nullptr, VQHIP_ERR_INVALID_ARG, "vqhip_create: device ordinal out of range");
    hipDeviceProp_t prop;
    HIP_TRY(nullptr, hipGetDeviceProperties(&prop, device_ordinal));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, VQHIP_ERR_NO_DEVICE, std::string("vqhip_create: device is ") + prop.gcnArchName + ", kernels are built for gfx950 only");
    HIP_TRY(nullptr, hipSetDevice(device_ordinal));
    vqhip_ctx* ctx = new vqhip_ctx();
    ctx->device = device_ordinal;
    ctx->nCUs = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    {
        int lds = 0;
        if (hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, device_ordinal) == hipSuccess && lds > 0) ctx->ldsPerBlock = lds;
    }
    ctx->generation = g_ctxGeneration.fetch_add(1, std::memory_order_relaxed);
    const size_t ringBytes = kConstSlotBytes * vqhip_ctx::kSlots;
    if ((e = hipHostMalloc((void**)&ctx->hostRing, ringBytes, hipHostMallocDefault)) != hipSuccess ||
        (e = hipMalloc((void**)&ctx->devRing, ringBytes)) != hipSuccess) {
        int rc = failHip(nullptr, e, "vqhip_create: constant ring allocation");
        vqhip_destroy(ctx);
        return rc;
    }
    for (int i = 0; i < vqhip_ctx::kLuts; ++i)
        if ((e = hipMalloc(&ctx->lut[i].table, 131072)) != hipSuccess || (e = hipEventCreateWithFlags(&ctx->lut[i].built, hipEventDisableTiming)) != hipSuccess ||
            (e = hipEventCreateWithFlags(&ctx->lut[i].lastUse, hipEventDisableTiming)) != hipSuccess) { int rc = failHip(nullptr, e, "vqhip_create: tonemap tables"); vqhip_destroy(ctx); return rc; }
    for (int i = 0; i < vqhip_ctx::kSlots; ++i)
        if ((e = hipEventCreateWithFlags(&ctx->slotEvent[i], hipEventDisableTiming)) != hipSuccess ||
            (e = hipEventCreateWithFlags(&ctx->copyEvent[i], hipEventDisableTiming)) != hipSuccess) { int rc = failHip(nullptr, e, "hipEventCreate"); vqhip_destroy(ctx); return rc; }
    if ((e = hipStreamCreateWithFlags(&ctx->copyStream, hipStreamNonBlocking)) != hipSuccess) { int rc = failHip(nullptr, e, "hipStreamCreate"); vqhip_destroy(ctx); return rc; }
    *out_ctx = ctx;
    return VQHIP_OK;
}

void vqhip_destroy(vqhip_ctx* ctx) {
    if (!ctx) return;
    if (g_lastErrorCtx == ctx) g_lastErrorCtx = nullptr;     // this thread's message dies with the context (other threads: the generation check)
    (void)hipSetDevice(ctx->device);
    (void)hipDeviceSynchronize();
    for (int i = 0; i < vqhip_ctx::kSlots; ++i) { if (ctx->slotEvent[i]) (void)hipEventDestroy(ctx->slotEvent[i]); if (ctx->copyEvent[i]) (void)hipEventDestroy(ctx->copyEvent[i]); }
    if (ctx->copyStream) (void)hipStreamDestroy(ctx->copyStream);
    if (ctx->hostRing) (void)hipHostFree(ctx->hostRing);
    if (ctx->devRing) (void)hipFree(ctx->devRing);
    if (ctx->scratch) (void)hipFree(ctx->scratch);
    if (ctx->rec) (void)hipFree(ctx->rec);
    if (ctx->recFree) (void)hipEventDestroy(ctx->recFree);
    if (ctx->edge) (void)hipFree(ctx->edge);
    if (ctx->edgeFree) (void)hipEventDestroy(ctx->edgeFree);
    if (ctx->hier) (void)hipFree(ctx->hier);
    if (ctx->hierFree) (void)hipEventDestroy(ctx->hierFree);
    if (ctx->ssrTiles) (void)hipFree(ctx->ssrTiles);
    if (ctx->ssrFree) (void)hipEventDestroy(ctx->ssrFree);
    for (int i = 0; i < vqhip_ctx::kLuts; ++i) {
        if (ctx->lut[i].table) (void)hipFree(ctx->lut[i].table);
        if (ctx->lut[i].built) (void)hipEventDestroy(ctx->lut[i].built);
        if (ctx->lut[i].lastUse) (void)hipEventDestroy(ctx->lut[i].lastUse);
    }
    delete ctx;
}

// validation of the lighting half shared by vqhip_forward_lighting and vqhip_forward_lighting_from_materials; *casters = shadow casters present
static int validateLighting(vqhip_ctx* ctx, const char* who, const VQ_PerFrameData* perFrame, const VQ_PerViewLightingData* perView,
                            const VQ_PointLight* extraPoint, int numExtraPoint, const vqhip_envmap* env, const vqhip_shadowmaps* sm, vqhip_format outFmt, bool* casters) {
    const std::string w(who);
    if (!perFrame || !perView) return fail(ctx, VQHIP_ERR_INVALID_ARG, w + ": NULL argument");
    if (!isImageFmt(outFmt)) return fail(ctx, VQHIP_ERR_UNSUPPORTED, w + ": outFmt must be RGBA32F or RGBA16F");
    const VQ_SceneLighting& L = perFrame->Lights;
    if (L.numPointLights < 0 || L.numPointLights > VQ_NUM_LIGHTS__POINT || L.numSpotLights < 0 || L.numSpotLights > VQ_NUM_LIGHTS__SPOT ||
        L.numPointCasters < 0 || L.numPointCasters > VQ_NUM_SHADOWING_LIGHTS__POINT || L.numSpotCasters < 0 || L.numSpotCasters > VQ_NUM_SHADOWING_LIGHTS__SPOT)
        return fail(ctx, VQHIP_ERR_INVALID_ARG, w + ": light count exceeds the cbuffer array (LightingConstantBufferData.h:39-44)");
    if (numExtraPoint < 0 || numExtraPoint > kMaxExtraPointLights || (numExtraPoint > 0 && !extraPoint))
        return fail(ctx, VQHIP_ERR_INVALID_ARG, w + ": bad extraPoint / numExtraPoint");
    *casters = L.numPointCasters > 0 || L.numSpotCasters > 0 || (L.directional.enabled && L.directional.shadowing);
    if (*casters) {
        if (!sm) return fail(ctx, VQHIP_ERR_INVALID_ARG, w + ": shadow casters present but sm is NULL");
        if ((L.numPointCasters > 0 && (!sm->point || sm->point_dim <= 0)) || (L.numSpotCasters > 0 && (!sm->spot || sm->spot_dim <= 0)) ||
            (L.directional.enabled && L.directional.shadowing && (!sm->directional || sm->dir_dim <= 0)))
            return fail(ctx, VQHIP_ERR_INVALID_ARG, w + ": missing shadow map for a caster");
        // the PCF kernels address a slice with 32-bit byte / texel offsets (vq_shade.h: pcf_2d, omni_pcf): 2-D maps up to 32768^2, cube faces up to 16384^2
        if ((L.numPointCasters > 0 && sm->point_dim > 16384) || (L.numSpotCasters > 0 && sm->spot_dim > 32768) ||
            (L.directional.enabled && L.directional.shadowing && sm->dir_dim > 32768))
            return fail(ctx, VQHIP_ERR_UNSUPPORTED, w + ": shadow map larger than 32768^2 (2-D) / 16384^2 (cube face)");
    }
    if (env) {
        if (!env->diffuse_cube || env->diffuse_res <= 0) return fail(ctx, VQHIP_ERR_INVALID_ARG, w + ": env->diffuse_cube missing");
        if (!perView->EnvironmentMapDiffuseOnlyIllumination &&
            (!env->specular_cube || env->spec_res0 <= 0 || env->spec_mips <= 0 || (env->spec_res0 >> (env->spec_mips - 1)) < 1 || !env->brdf_lut || env->lut_size <= 0))
            return fail(ctx, VQHIP_ERR_INVALID_ARG, w + ": env specular cube / BRDF LUT missing");
    }
    return VQHIP_OK;
}
// the lighting pass's constant block (cbuffers b0 / b1 + descriptors + the packed point-light records) into a ring slot; returns its byte size
static size_t fillFrameConstants(vqhip_ctx* ctx, int slot, const VQ_PerFrameData* perFrame, const VQ_PerViewLightingData* perView,
                                 const VQ_PointLight* extraPoint, int numExtraPoint, const vqhip_envmap* env, const vqhip_shadowmaps* sm) {
    const VQ_SceneLighting& L = perFrame->Lights;
    FrameConstants* fc = (FrameConstants*)(ctx->hostRing + (size_t)slot * kConstSlotBytes);
    std::memset(fc, 0, sizeof(FrameConstants));
    fc->perFrame = *perFrame;
    fc->perView = *perView;
    if (env) fc->env = *env;
    if (sm) fc->sm = *sm;
    fc->hasEnv = env ? 1 : 0;
    fc->pow5ExpLog = ctx->pow5ExpLog;
    // GetHDRIRotationMatrix, Lighting.hlsl:348-358: a per-frame constant (the shader's own TODO: "pass m with cbuffer") — sin / cos are taken
    // correctly rounded (double libm rounded to float), like the oracle; the contract's polynomial cos is 1 ulp off at e.g. 0.3 rad
    fc->hdriSin = (float)std::sin((double)-perFrame->fHDRIOffsetInRadians);
    fc->hdriCos = (float)std::cos((double)-perFrame->fHDRIOffsetInRadians);
    // pack the non-shadowing point lights for the hot loop: cbuffer array first, then the extension array, in index order
    DevPointLight* pts = (DevPointLight*)(fc + 1);
    const int nPts = L.numPointLights + numExtraPoint;
    int32_t pointFastOK = 1, pointSkipOK = 1, negZeroAxes = 0;
    auto coordOK = [](float c) { const float m = std::fabs(c); return c == 0.0f || (m >= 0x1p-40f && m <= 0x1p40f); };      // false for NaN / inf
    for (int i = 0; i < nPts; ++i) {
        const VQ_PointLight& l = i < L.numPointLights ? L.point_lights[i] : extraPoint[i - L.numPointLights];
        pts[i].px = l.position.x; pts[i].py = l.position.y; pts[i].pz = l.position.z; pts[i].range = l.range;
        pts[i].cbx = l.color.x * l.brightness; pts[i].cby = l.color.y * l.brightness; pts[i].cbz = l.color.z * l.brightness;   // l.color * l.brightness (Lighting.hlsl:317)
        pts[i].rangeSq = rangeCullThreshold(l.range);
        if (pts[i].rangeSq > 0x1p60f) pointFastOK = 0;                           // false for a NaN threshold (never lit)
        // the light loop proves its fast quotients from the GRANULARITY of the coordinates (vq_shade.h:add_point_light): a non-zero Lw - P then has magnitude >= 2^-63
        if (!(coordOK(l.position.x) && coordOK(l.position.y) && coordOK(l.position.z))) pointFastOK = 0;
        if (l.position.x == 0.0f && std::signbit(l.position.x)) negZeroAxes |= 1;
        if (l.position.y == 0.0f && std::signbit(l.position.y)) negZeroAxes |= 2;
        if (l.position.z == 0.0f && std::signbit(l.position.z)) negZeroAxes |= 4;
        if (!(std::isfinite(pts[i].cbx) && std::isfinite(pts[i].cby) && std::isfinite(pts[i].cbz))) pointSkipOK = 0;
    }
    // spot / directional lights: the wave-uniform parts of SpotlightIntensity / CalculateDirectionalLightIllumination, with the shader's own operations
    // (this translation unit is built with -ffp-contract=off: every product and sum below is rounded on its own)
    const bool dxc = ctx->arithDxc != 0;
    auto normalizeAsShader = [dxc](const VQ_float3& v, float* o) {
        if (dxc) {                                                               // DXC reading: v * rsqrt(dot(v, v)), FMA-chain dot, correctly rounded rsqrt (vq_devmath.h:rsqrt_cr)
            const float dd = std::fma(v.z, v.z, std::fma(v.y, v.y, v.x * v.x));
            const float r = (float)(1.0 / std::sqrt((double)dd));
            o[0] = v.x * r; o[1] = v.y * r; o[2] = v.z * r;
        } else {                                                                 // literal reading: one IEEE quotient per component by length(v)
            const float dd = (v.x * v.x + v.y * v.y) + v.z * v.z;
            const float D = std::sqrt(dd);
            o[0] = v.x / D; o[1] = v.y / D; o[2] = v.z / D;
        }
    };
    for (int i = 0; i < VQ_NUM_LIGHTS__SPOT + VQ_NUM_SHADOWING_LIGHTS__SPOT; ++i) {
        const bool caster = i >= VQ_NUM_LIGHTS__SPOT;
        if (i >= (caster ? VQ_NUM_LIGHTS__SPOT + L.numSpotCasters : L.numSpotLights)) continue;
        const VQ_SpotLight& l = caster ? L.spot_casters[i - VQ_NUM_LIGHTS__SPOT] : L.spot_lights[i];
        DevSpotLight& ds = fc->spot[i];
        float sd[3];
        normalizeAsShader(l.spotDir, sd);
        ds.sdx = sd[0]; ds.sdy = sd[1]; ds.sdz = sd[2];
        const float den = l.outerConeAngle - l.innerConeAngle;
        ds.rConeDen = 1.0f / den;
        ds.cbx = l.color.x * l.brightness; ds.cby = l.color.y * l.brightness; ds.cbz = l.color.z * l.brightness;
        ds.flags = ((std::isnormal(den) && std::isnormal(ds.rConeDen)) ? 1 : 0) | ((std::isfinite(ds.cbx) && std::isfinite(ds.cby) && std::isfinite(ds.cbz)) ? 2 : 0);
    }
    {
        const VQ_float3 nd = { -L.directional.lightDirection.x, -L.directional.lightDirection.y, -L.directional.lightDirection.z };
        normalizeAsShader(nd, fc->dirWi);
    }
    fc->pointFastOK = pointFastOK;
    fc->pointSkipOK = pointSkipOK;
    fc->pointNegZeroAxes = negZeroAxes;
    fc->numPointAll = nPts;
    return sizeof(FrameConstants) + (size_t)nPts * sizeof(DevPointLight);
}

// vqhip_psmain_targets -> kernel arguments; NULL / no output bound: all-zero (the kernels then touch nothing)
static int fillMrt(vqhip_ctx* ctx, const char* who, const vqhip_psmain_targets* t, int width, MrtArgs* m) {
    std::memset(m, 0, sizeof(*m));
    if (!t || (!t->albedo_metallic && !t->motion_vectors)) return VQHIP_OK;
    const std::string w(who);
    if (t->albedo_metallic) {
        if (t->albedo_fmt != VQHIP_FMT_RGBA16F && t->albedo_fmt != VQHIP_FMT_RGBA32F) return fail(ctx, VQHIP_ERR_UNSUPPORTED, w + ": albedo_fmt must be RGBA16F or RGBA32F");
        m->albedoPitch = t->albedo_pitch_px ? t->albedo_pitch_px : width;
        if (m->albedoPitch < width) return fail(ctx, VQHIP_ERR_INVALID_ARG, w + ": albedo_pitch_px below the width");
        m->albedo = t->albedo_metallic; m->albedoF32 = t->albedo_fmt == VQHIP_FMT_RGBA32F;
    }
    if (t->motion_vectors) {
        if (t->motion_fmt != VQHIP_FMT_RG16F && t->motion_fmt != VQHIP_FMT_RG32F) return fail(ctx, VQHIP_ERR_UNSUPPORTED, w + ": motion_fmt must be RG16F or RG32F");
        if (!t->svPositionCurr || !t->svPositionPrev) return fail(ctx, VQHIP_ERR_INVALID_ARG, w + ": motion_vectors needs svPositionCurr and svPositionPrev");
        m->motionPitch = t->motion_pitch_px ? t->motion_pitch_px : width;
        m->svPitch = t->sv_pitch_px ? t->sv_pitch_px : width;
        if (m->motionPitch < width || m->svPitch < width) return fail(ctx, VQHIP_ERR_INVALID_ARG, w + ": motion_pitch_px / sv_pitch_px below the width");
        m->motion = t->motion_vectors; m->motionF32 = t->motion_fmt == VQHIP_FMT_RG32F;
        m->svCurr = (const float4*)t->svPositionCurr; m->svPrev = (const float4*)t->svPositionPrev;
    }
    return VQHIP_OK;
}

// vqhip_forward_lighting (targets == NULL) and its _mrt form
static int forwardLighting(vqhip_ctx* ctx, void* stream, const vqhip_gbuffer* gb, const VQ_PerFrameData* perFrame, const VQ_PerViewLightingData* perView,
        const VQ_PointLight* extraPoint, int numExtraPoint, const vqhip_envmap* env, const vqhip_shadowmaps* sm,
        void* out, int out_row_pitch_px, vqhip_format outFmt, const vqhip_psmain_targets* targets) {
    vqk::Range range_("RenderSceneColor");
    ShadeArgs a;
    if (!gb || !perFrame || !perView || !out) return fail(ctx, VQHIP_ERR_INVALID_ARG, "forward_lighting: NULL argument");
    if (!gbufferPlanes(*gb, &a)) return fail(ctx, VQHIP_ERR_INVALID_ARG, "forward_lighting: NULL G-buffer plane");
    if (gb->width <= 0 || gb->height <= 0 || gb->row_pitch_px < gb->width || out_row_pitch_px < gb->width)
        return fail(ctx, VQHIP_ERR_INVALID_ARG, "forward_lighting: bad dimensions / pitch");
    bool casters = false;
    int rc = validateLighting(ctx, "forward_lighting", perFrame, perView, extraPoint, numExtraPoint, env, sm, outFmt, &casters);
    if (rc) return rc;
    if ((rc = fillMrt(ctx, "forward_lighting", targets, gb->width, &a.mrt)) != VQHIP_OK) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    int slot;
    if ((rc = stageConstants(ctx, st, &slot, &a.fc, fillFrameConstants, perFrame, perView, extraPoint, numExtraPoint, env, sm)) != VQHIP_OK) return rc;
    a.out = out;
    a.width = gb->width; a.height = gb->height; a.pitch = gb->row_pitch_px; a.outPitch = out_row_pitch_px;
    a.arithDxc = ctx->arithDxc;
    hipError_t e = launch_forward_lighting(st, a, env != nullptr, casters, outFmt, ctx->opt);
    if (e != hipSuccess) return failHip(ctx, e, "forward_lighting launch");
    return releaseSlot(ctx, slot, st);
}
int vqhip_forward_lighting(vqhip_ctx* ctx, void* stream, const vqhip_gbuffer* gb,
        const VQ_PerFrameData* perFrame, const VQ_PerViewLightingData* perView,
        const VQ_PointLight* extraPoint, int numExtraPoint,
        const vqhip_envmap* env, const vqhip_shadowmaps* sm,
        void* out, int out_row_pitch_px, vqhip_format outFmt) {
    if (!ctx) return fail(nullptr, VQHIP_ERR_INVALID_ARG, "forward_lighting: ctx is NULL");
    CTX_GUARD(ctx, "forward_lighting");
    return forwardLighting(ctx, stream, gb, perFrame, perView, extraPoint, numExtraPoint, env, sm, out, out_row_pitch_px, outFmt, nullptr);
}
int vqhip_forward_lighting_mrt(vqhip_ctx* ctx, void* stream, const vqhip_gbuffer* gb,
        const VQ_PerFrameData* perFrame, const VQ_PerViewLightingData* perView,
        const VQ_PointLight* extraPoint, int numExtraPoint,
        const vqhip_envmap* env, const vqhip_shadowmaps* sm,
        void* out, int out_row_pitch_px, vqhip_format outFmt, const vqhip_psmain_targets* targets) {
    if (!ctx) return fail(nullptr, VQHIP_ERR_INVALID_ARG, "forward_lighting: ctx is NULL");
    CTX_GUARD(ctx, "forward_lighting");
    return forwardLighting(ctx, stream, gb, perFrame, perView, extraPoint, numExtraPoint, env, sm, out, out_row_pitch_px, outFmt, targets);
}

int vqhip_forward_lighting_msaa(vqhip_ctx* ctx, void* stream, const vqhip_gbuffer_msaa* gb,
        const VQ_PerFrameData* perFrame, const VQ_PerViewLightingData* perView,
        const VQ_PointLight* extraPoint, int numExtraPoint,
        const vqhip_envmap* env, const vqhip_shadowmaps* sm,
        const void* background, int background_pitch_px,
        void* out, int out_row_pitch_px, vqhip_format outFmt) {
    vqk::Range range_("RenderSceneColor");
    if (!ctx) return fail(nullptr, VQHIP_ERR_INVALID_ARG, "forward_lighting_msaa: ctx is NULL");
    CTX_GUARD(ctx, "forward_lighting_msaa");
    if (!gb || !out) return fail(ctx, VQHIP_ERR_INVALID_ARG, "forward_lighting_msaa: NULL argument");
    if (gb->layers < 1 || gb->layers > VQHIP_MSAA_MAX_LAYERS) return fail(ctx, VQHIP_ERR_INVALID_ARG, "forward_lighting_msaa: layers must be 1..4");
    const int W = gb->layer[0].width, H = gb->layer[0].height;
    if (W <= 0 || H <= 0) return fail(ctx, VQHIP_ERR_INVALID_ARG, "forward_lighting_msaa: bad dimensions");
    if ((uint64_t)W * (uint64_t)H > 0xFFFFFFFFull) return fail(ctx, VQHIP_ERR_UNSUPPORTED, "forward_lighting_msaa: more than 2^32 - 1 pixels");
    const int covPitch = gb->coverage_pitch ? gb->coverage_pitch : W;
    if (covPitch < W || out_row_pitch_px < W || (background && background_pitch_px < W))
        return fail(ctx, VQHIP_ERR_INVALID_ARG, "forward_lighting_msaa: pitch below the width");
    if (background && background == out) return fail(ctx, VQHIP_ERR_INVALID_ARG, "forward_lighting_msaa: background must not be out");
    MsaaArgs a;
    std::memset(&a, 0, sizeof(a));
    for (int k = 0; k < gb->layers; ++k) {
        const vqhip_gbuffer& g = gb->layer[k];
        if (!gbufferPlanes(g, &a.L[k]) || !gb->coverage[k])
            return fail(ctx, VQHIP_ERR_INVALID_ARG, "forward_lighting_msaa: NULL plane or coverage of layer " + std::to_string(k));
        if (g.width != W || g.height != H) return fail(ctx, VQHIP_ERR_INVALID_ARG, "forward_lighting_msaa: layers of different sizes");
        if (g.row_pitch_px < W) return fail(ctx, VQHIP_ERR_INVALID_ARG, "forward_lighting_msaa: pitch below the width");
        a.L[k].cov = gb->coverage[k]; a.L[k].pitch = g.row_pitch_px;
    }
    bool casters = false;
    int rc = validateLighting(ctx, "forward_lighting_msaa", perFrame, perView, extraPoint, numExtraPoint, env, sm, outFmt, &casters);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    // the edge list: the previous call's kernels (maybe on another stream) are done with it before this stream touches it
    const size_t edgeNeed = 4 + 4 * (size_t)W * (size_t)H;
    if (ctx->edgeUsed) HIP_TRY(ctx, hipStreamWaitEvent(st, ctx->edgeFree, 0));
    if (ctx->edgeBytes < edgeNeed) {
        if (ctx->edge) { HIP_TRY(ctx, hipDeviceSynchronize()); HIP_TRY(ctx, hipFree(ctx->edge)); ctx->edge = nullptr; ctx->edgeBytes = 0; }
        HIP_TRY(ctx, hipMalloc(&ctx->edge, edgeNeed));
        ctx->edgeBytes = edgeNeed;
    }
    if (!ctx->edgeFree) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->edgeFree, hipEventDisableTiming));
    int slot;
    if ((rc = stageConstants(ctx, st, &slot, &a.fc, fillFrameConstants, perFrame, perView, extraPoint, numExtraPoint, env, sm)) != VQHIP_OK) return rc;
    a.bg = background; a.out = out;
    a.edgeCount = (uint32_t*)ctx->edge; a.edgeList = (uint32_t*)ctx->edge + 1;
    a.width = W; a.height = H; a.layers = gb->layers; a.covPitch = covPitch; a.bgPitch = background_pitch_px; a.outPitch = out_row_pitch_px;
    HIP_TRY(ctx, hipMemsetAsync(ctx->edge, 0, 4, st));
    hipError_t e = launch_forward_lighting_msaa(st, a, env != nullptr, casters, outFmt, ctx->arithDxc, ctx->nCUs, ctx->opt);
    if (e != hipSuccess) return failHip(ctx, e, "forward_lighting_msaa launch");
    HIP_TRY(ctx, hipEventRecord(ctx->edgeFree, st));
    ctx->edgeUsed = true;
    return releaseSlot(ctx, slot, st);
}

int vqhip_gaussian_blur_x(vqhip_ctx* ctx, void* stream, const void* in, void* out, const VQ_BlurParams* p, vqhip_format fmt) {
    vqk::Range range_("BlurX");
    if (!ctx) return fail(nullptr, VQHIP_ERR_INVALID_ARG, "gaussian_blur_x: ctx is NULL");
    CTX_GUARD(ctx, "gaussian_blur_x");
    if (!in || !out || !p || p->iImageSizeX <= 0 || p->iImageSizeY <= 0) return fail(ctx, VQHIP_ERR_INVALID_ARG, "gaussian_blur_x: bad argument");
    if (!isImageFmt(fmt)) return fail(ctx, VQHIP_ERR_UNSUPPORTED, "gaussian_blur_x: fmt must be RGBA32F or RGBA16F");
    if (in == out) return fail(ctx, VQHIP_ERR_INVALID_ARG, "gaussian_blur_x: in-place blur is not supported");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipError_t e = launch_blur_x((hipStream_t)stream, in, out, p->iImageSizeX, p->iImageSizeY, fmt, ctx->opt);
    return e == hipSuccess ? VQHIP_OK : failHip(ctx, e, "blur_x launch");
}

int vqhip_gaussian_blur_y(vqhip_ctx* ctx, void* stream, const void* in, void* out, const void* halo_top, const void* halo_bottom, int halo_rows,
                          const VQ_BlurParams* p, vqhip_format fmt) {
    vqk::Range range_("BlurY");
    if (!ctx) return fail(nullptr, VQHIP_ERR_INVALID_ARG, "gaussian_blur_y: ctx is NULL");
    CTX_GUARD(ctx, "gaussian_blur_y");
    if (!in || !out || !p || p->iImageSizeX <= 0 || p->iImageSizeY <= 0) return fail(ctx, VQHIP_ERR_INVALID_ARG, "gaussian_blur_y: bad argument");
    if (!isImageFmt(fmt)) return fail(ctx, VQHIP_ERR_UNSUPPORTED, "gaussian_blur_y: fmt must be RGBA32F or RGBA16F");
    if (in == out) return fail(ctx, VQHIP_ERR_INVALID_ARG, "gaussian_blur_y: in-place blur is not supported");
    if ((halo_top || halo_bottom) && halo_rows < 10) return fail(ctx, VQHIP_ERR_INVALID_ARG, "gaussian_blur_y: halo_rows must be >= 10 (KERNEL_RANGE-1)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipError_t e = launch_blur_y((hipStream_t)stream, in, out, halo_top, halo_bottom, halo_rows, p->iImageSizeX, p->iImageSizeY, fmt);
    return e == hipSuccess ? VQHIP_OK : failHip(ctx, e, "blur_y launch");
}

int vqhip_gaussian_blur_y_tonemap(vqhip_ctx* ctx, void* stream, const void* in, void* out, const void* halo_top, const void* halo_bottom, int halo_rows,
                                  const VQ_BlurParams* p, const VQ_TonemapperParams* tm, vqhip_format blurFmt, vqhip_format outFmt) {
    vqk::Range range_("BlurY+TonemapperCS");
    if (!ctx) return fail(nullptr, VQHIP_ERR_INVALID_ARG, "gaussian_blur_y_tonemap: ctx is NULL");
    CTX_GUARD(ctx, "gaussian_blur_y_tonemap");
    if (!in || !out || !p || !tm || p->iImageSizeX <= 0 || p->iImageSizeY <= 0) return fail(ctx, VQHIP_ERR_INVALID_ARG, "gaussian_blur_y_tonemap: bad argument");
    if (!isImageFmt(blurFmt)) return fail(ctx, VQHIP_ERR_UNSUPPORTED, "gaussian_blur_y_tonemap: blurFmt must be RGBA32F or RGBA16F");
    if (!isImageFmt(outFmt) && outFmt != VQHIP_FMT_RGBA8_UNORM) return fail(ctx, VQHIP_ERR_UNSUPPORTED, "gaussian_blur_y_tonemap: outFmt must be RGBA32F, RGBA16F or RGBA8_UNORM");
    if (in == out) return fail(ctx, VQHIP_ERR_INVALID_ARG, "gaussian_blur_y_tonemap: in-place is not supported");
    if ((halo_top || halo_bottom) && halo_rows < 10) return fail(ctx, VQHIP_ERR_INVALID_ARG, "gaussian_blur_y_tonemap: halo_rows must be >= 10");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int slot = -1;
    if (blur_y_tonemap_uses_lut(*tm, blurFmt, outFmt, (size_t)p->iImageSizeX * p->iImageSizeY)) { const int rc = acquireTonemapLut(ctx, (hipStream_t)stream, *tm, outFmt, &slot); if (rc) return rc; }
    hipError_t e = launch_blur_y_tonemap((hipStream_t)stream, in, out, halo_top, halo_bottom, halo_rows, p->iImageSizeX, p->iImageSizeY, *tm, blurFmt, outFmt,
                                         slot >= 0 ? ctx->lut[slot].table : nullptr, ctx->opt);
    if (e != hipSuccess) return failHip(ctx, e, "blur_y_tonemap launch");
    return slot >= 0 ? releaseTonemapLut(ctx, (hipStream_t)stream, slot) : VQHIP_OK;
}

int vqhip_gaussian_blur(vqhip_ctx* ctx, void* stream, const void* in, void* tmp, void* out, const VQ_BlurParams* p, vqhip_format fmt) {
    if (!ctx) return fail(nullptr, VQHIP_ERR_INVALID_ARG, "gaussian_blur: ctx is NULL");
    CTX_GUARD(ctx, "gaussian_blur");
    if (!tmp) return fail(ctx, VQHIP_ERR_INVALID_ARG, "gaussian_blur: tmp is NULL");
    int rc = vqhip_gaussian_blur_x(ctx, stream, in, tmp, p, fmt);
    if (rc) return rc;
    return vqhip_gaussian_blur_y(ctx, stream, tmp, out, nullptr, nullptr, 0, p, fmt);
}

int vqhip_tonemap(vqhip_ctx* ctx, void* stream, const void* in, void* out, int width, int height,
                  const VQ_TonemapperParams* p, vqhip_format inFmt, vqhip_format outFmt) {
    vqk::Range range_("TonemapperCS");
    if (!ctx) return fail(nullptr, VQHIP_ERR_INVALID_ARG, "tonemap: ctx is NULL");
    CTX_GUARD(ctx, "tonemap");
    if (!in || !out || !p || width <= 0 || height <= 0) return fail(ctx, VQHIP_ERR_INVALID_ARG, "tonemap: bad argument");
    if (!isImageFmt(inFmt)) return fail(ctx, VQHIP_ERR_UNSUPPORTED, "tonemap: inFmt must be RGBA32F or RGBA16F");
    if (!isImageFmt(outFmt) && outFmt != VQHIP_FMT_RGBA8_UNORM) return fail(ctx, VQHIP_ERR_UNSUPPORTED, "tonemap: outFmt must be RGBA32F, RGBA16F or RGBA8_UNORM");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int slot = -1;
    if (tonemap_uses_lut(*p, inFmt, outFmt, (size_t)width * height)) { const int rc = acquireTonemapLut(ctx, (hipStream_t)stream, *p, outFmt, &slot); if (rc) return rc; }
    hipError_t e = launch_tonemap((hipStream_t)stream, in, out, width, height, *p, inFmt, outFmt, slot >= 0 ? ctx->lut[slot].table : nullptr, ctx->opt);
    if (e != hipSuccess) return failHip(ctx, e, "tonemap launch");
    return slot >= 0 ? releaseTonemapLut(ctx, (hipStream_t)stream, slot) : VQHIP_OK;
}

// sceneColor -> out for one row tile; halo_top / halo_bottom are SCENE-COLOUR rows (NULL: image border)
static int postProcessTile(vqhip_ctx* ctx, void* stream, const void* sceneColor, void* out, const void* halo_top, const void* halo_bottom, int halo_rows,
                           int width, int height, const VQ_TonemapperParams* tm, vqhip_format inFmt, vqhip_format outFmt) {
    const hipStream_t st = (hipStream_t)stream;
    if (post_chain_applies(*tm, inFmt, outFmt, width, height, ctx->opt)) {                      // X, Y and the tonemapper in one kernel: no intermediate at all
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        int slot = -1;
        const int rc = acquireTonemapLut(ctx, st, *tm, outFmt, &slot);
        if (rc) return rc;
        hipError_t e = launch_post_chain(st, sceneColor, out, halo_top, halo_bottom, halo_rows, width, height, ctx->lut[slot].table, ctx->nCUs, ctx->opt);
        if (e != hipSuccess) return failHip(ctx, e, "post chain launch");
        return releaseTonemapLut(ctx, st, slot);
    }
    // blur X into a BlurIntermediate held in the context's scratch buffer (the tile, then the halo rows behind it), then blur Y + tonemap in one kernel
    // (or on the LDS-tile kernel: HDR / RGBA32F targets)
    const size_t bpp = inFmt == VQHIP_FMT_RGBA32F ? 16 : 8;
    const size_t tileBytes = (size_t)width * height * bpp, haloBytes = (size_t)width * halo_rows * bpp;
    const int rc0 = ensureScratch(ctx, tileBytes + 2 * haloBytes);
    if (rc0) return rc0;
    char* xt = (char*)ctx->scratch; char* xTop = xt + tileBytes; char* xBot = xTop + haloBytes;
    const VQ_BlurParams bp = { width, height };
    int rc = vqhip_gaussian_blur_x(ctx, stream, sceneColor, xt, &bp, inFmt);
    if (rc) return rc;
    const VQ_BlurParams hp = { width, halo_rows };
    if (halo_top && (rc = vqhip_gaussian_blur_x(ctx, stream, halo_top, xTop, &hp, inFmt))) return rc;
    if (halo_bottom && (rc = vqhip_gaussian_blur_x(ctx, stream, halo_bottom, xBot, &hp, inFmt))) return rc;
    return vqhip_gaussian_blur_y_tonemap(ctx, stream, xt, out, halo_top ? xTop : nullptr, halo_bottom ? xBot : nullptr, halo_rows, &bp, tm, inFmt, outFmt);
}

static int postProcessCheck(vqhip_ctx* ctx, const char* who, const void* sceneColor, const void* out, int width, int height, const VQ_TonemapperParams* tm,
                            vqhip_format inFmt, vqhip_format outFmt) {
    const std::string w = who;
    if (!sceneColor || !out || !tm || width <= 0 || height <= 0) return fail(ctx, VQHIP_ERR_INVALID_ARG, w + ": bad argument");
    if (!isImageFmt(inFmt)) return fail(ctx, VQHIP_ERR_UNSUPPORTED, w + ": inFmt must be RGBA32F or RGBA16F");
    if (!isImageFmt(outFmt) && outFmt != VQHIP_FMT_RGBA8_UNORM) return fail(ctx, VQHIP_ERR_UNSUPPORTED, w + ": outFmt must be RGBA32F, RGBA16F or RGBA8_UNORM");
    if (sceneColor == out) return fail(ctx, VQHIP_ERR_INVALID_ARG, w + ": in-place is not supported");
    return VQHIP_OK;
}

int vqhip_post_process(vqhip_ctx* ctx, void* stream, const void* sceneColor, void* out, int width, int height,
                       const VQ_TonemapperParams* tm, int enableGaussianBlur, vqhip_format inFmt, vqhip_format outFmt) {
    vqk::Range range_("RenderPostProcess");
    if (!ctx) return fail(nullptr, VQHIP_ERR_INVALID_ARG, "post_process: ctx is NULL");
    CTX_GUARD(ctx, "post_process");
    const int rc = postProcessCheck(ctx, "post_process", sceneColor, out, width, height, tm, inFmt, outFmt);
    if (rc) return rc;
    if (!enableGaussianBlur) return vqhip_tonemap(ctx, stream, sceneColor, out, width, height, tm, inFmt, outFmt);
    return postProcessTile(ctx, stream, sceneColor, out, nullptr, nullptr, 0, width, height, tm, inFmt, outFmt);
}

int vqhip_post_process_tile(vqhip_ctx* ctx, void* stream, const void* sceneColor, void* out, const void* halo_top, const void* halo_bottom, int halo_rows,
                            int width, int height, const VQ_TonemapperParams* tm, vqhip_format inFmt, vqhip_format outFmt) {
    vqk::Range range_("RenderPostProcess(tile)");
    if (!ctx) return fail(nullptr, VQHIP_ERR_INVALID_ARG, "post_process_tile: ctx is NULL");
    CTX_GUARD(ctx, "post_process_tile");
    const int rc = postProcessCheck(ctx, "post_process_tile", sceneColor, out, width, height, tm, inFmt, outFmt);
    if (rc) return rc;
    if ((halo_top || halo_bottom) && halo_rows < 10) return fail(ctx, VQHIP_ERR_INVALID_ARG, "post_process_tile: halo_rows must be >= 10");
    if (!halo_top && !halo_bottom) halo_rows = 0;
    return postProcessTile(ctx, stream, sceneColor, out, halo_top, halo_bottom, halo_rows, width, height, tm, inFmt, outFmt);
}

int vqhip_set_option(vqhip_ctx* ctx, const char* key, const char* value) {
    if (!ctx) return fail(nullptr, VQHIP_ERR_INVALID_ARG, "set_option: ctx is NULL");
    CTX_GUARD(ctx, "set_option");
    if (!key) return fail(ctx, VQHIP_ERR_INVALID_ARG, "set_option: key is NULL");
    const std::string k = key, v = (value && std::strcmp(value, "default")) ? value : "";
    vqk::Options& o = ctx->opt;
    auto num = [&](int* dst, std::initializer_list<int> allowed) -> int {       // "" -> 0 (default); otherwise a non-negative integer (from `allowed` when given)
        if (v.empty()) { *dst = 0; return VQHIP_OK; }
        char* end = nullptr;
        const long n = std::strtol(v.c_str(), &end, 10);
        bool ok = end && !*end && n >= 0 && n <= (1 << 24);
        if (ok && allowed.size()) { ok = false; for (int a : allowed) ok |= a == (int)n; }
        if (!ok) return fail(ctx, VQHIP_ERR_INVALID_ARG, "set_option: bad value '" + v + "' for " + k);
        *dst = (int)n; return VQHIP_OK;
    };
    auto pick = [&](int* dst, std::initializer_list<const char*> names) -> int {  // names[i] selects value i + 1
        if (v.empty()) { *dst = 0; return VQHIP_OK; }
        int i = 1;
        for (const char* n : names) { if (v == n) { *dst = i; return VQHIP_OK; } ++i; }
        return fail(ctx, VQHIP_ERR_INVALID_ARG, "set_option: bad value '" + v + "' for " + k);
    };
    if (k == "shade_wg") return num(&o.shadeWg, { 0, 64, 128, 256 });
    if (k == "psmain_waves") return num(&o.psmainWaves, { 0, 4, 5, 6 });
    if (k == "blur_y_wgs") return num(&o.blurYWgs, {});
    if (k == "msaa_edge_wgs") return num(&o.msaaEdgeWgs, {});
    if (k == "post_form") return pick(&o.postForm, { "two", "chain" });
    if (k == "post_strips") return num(&o.postStrips, {});
    if (k == "lut_form") return pick(&o.lutForm, { "general" });
    if (k == "specular_form") return pick(&o.specularForm, { "general" });
    if (k == "diffuse_form") { if (v == "records") { o.diffuseForm = 0; return VQHIP_OK; } return pick(&o.diffuseForm, { "texels", "general" }); }
    if (k == "diffuse_seq_form") { if (v == "ordered") { o.diffuseSeqForm = 0; return VQHIP_OK; } return pick(&o.diffuseSeqForm, { "lane" }); }
    if (k == "raster_tile") return num(&o.rasterTile, { 0, 32, 64 });
    if (k == "interp_form") return pick(&o.interpForm, { "lane", "wave" });
    return fail(ctx, VQHIP_ERR_INVALID_ARG, "set_option: unknown key '" + k + "'");
}
int vqhip_set_arithmetic(vqhip_ctx* ctx, vqhip_arithmetic mode) {
    if (!ctx) return fail(nullptr, VQHIP_ERR_INVALID_ARG, "set_arithmetic: ctx is NULL");
    CTX_GUARD(ctx, "set_arithmetic");
    if (mode != VQHIP_ARITH_LITERAL && mode != VQHIP_ARITH_DXC) return fail(ctx, VQHIP_ERR_INVALID_ARG, "set_arithmetic: unknown mode");
    ctx->arithDxc = mode == VQHIP_ARITH_DXC ? 1 : 0;
    return VQHIP_OK;
}
int vqhip_set_fresnel_pow(vqhip_ctx* ctx, vqhip_fresnel_pow mode) {
    if (!ctx) return fail(nullptr, VQHIP_ERR_INVALID_ARG, "set_fresnel_pow: ctx is NULL");
    CTX_GUARD(ctx, "set_fresnel_pow");
    if (mode != VQHIP_FRESNEL_POW_PRODUCT && mode != VQHIP_FRESNEL_POW_EXP2_LOG2) return fail(ctx, VQHIP_ERR_INVALID_ARG, "set_fresnel_pow: unknown mode");
    ctx->pow5ExpLog = mode == VQHIP_FRESNEL_POW_EXP2_LOG2 ? 1 : 0;
    return VQHIP_OK;
}

int vqhip_brdf_lut(vqhip_ctx* ctx, void* stream, void* outRG, int size, int samples, vqhip_format fmt) {
    vqk::Range range_("CreateBRDFIntegralLUT");
    if (!ctx) return fail(nullptr, VQHIP_ERR_INVALID_ARG, "brdf_lut: ctx is NULL");
    CTX_GUARD(ctx, "brdf_lut");
    if (!outRG || size <= 0 || samples <= 0) return fail(ctx, VQHIP_ERR_INVALID_ARG, "brdf_lut: bad argument");
    if (fmt != VQHIP_FMT_RG16F && fmt != VQHIP_FMT_RG32F) return fail(ctx, VQHIP_ERR_UNSUPPORTED, "brdf_lut: fmt must be RG16F or RG32F");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipError_t e = launch_brdf_lut((hipStream_t)stream, outRG, size, samples, fmt, ctx->pow5ExpLog, ctx->opt);
    return e == hipSuccess ? VQHIP_OK : failHip(ctx, e, "brdf_lut launch");
}

int vqhip_mip_level_count(int w, int h) { int m = w > h ? w : h; if (m < 1) return 0; int n = 1; while (m > 1) { m >>= 1; ++n; } return n; }
size_t vqhip_mip_level_offset_bytes(int w0, int h0, int level) {
    size_t off = 0;
    for (int l = 0; l < level; ++l) off += (size_t)mipDim(w0, l) * mipDim(h0, l) * 16;
    return off;
}
size_t vqhip_mip_chain_bytes(int w0, int h0, int nMips) { return vqhip_mip_level_offset_bytes(w0, h0, nMips); }

int vqhip_mip_chain_min_rgba32f(vqhip_ctx* ctx, void* stream, void* mips, int w0, int h0, int nMips) {
    vqk::Range range_("GenerateMips");
    if (!ctx) return fail(nullptr, VQHIP_ERR_INVALID_ARG, "mip_chain: ctx is NULL");
    CTX_GUARD(ctx, "mip_chain");
    if (!mips || w0 <= 0 || h0 <= 0 || nMips <= 0 || nMips > vqhip_mip_level_count(w0, h0)) return fail(ctx, VQHIP_ERR_INVALID_ARG, "mip_chain: bad argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    for (int l = 1; l < nMips; ++l) {
        const float4* src = (const float4*)((const char*)mips + vqhip_mip_level_offset_bytes(w0, h0, l - 1));
        float4* dst = (float4*)((char*)mips + vqhip_mip_level_offset_bytes(w0, h0, l));
        hipError_t e = launch_mip_min((hipStream_t)stream, src, dst, mipDim(w0, l - 1), mipDim(h0, l - 1), mipDim(w0, l), mipDim(h0, l));
        if (e != hipSuccess) return failHip(ctx, e, "mip_min launch");
    }
    return VQHIP_OK;
}

// ---- 4x MSAA surface resolve + depth hierarchy (depth.hip; docs/DESIGN_DETAILS.md §7.10) ------------------------------------------------
static size_t depthLevelOffsetFloats(int w, int h, int level) {
    size_t off = 0;
    for (int l = 0; l < level; ++l) off += (size_t)mipDim(w, l) * mipDim(h, l);
    return off;
}
size_t vqhip_depth_hierarchy_level_offset_bytes(int width, int height, int level) {
    if (width <= 0 || height <= 0 || level < 0) return 0;
    const int L = vqhip_mip_level_count(width, height);
    return depthLevelOffsetFloats(width, height, level < L ? level : L) * 4;
}
size_t vqhip_depth_hierarchy_bytes(int width, int height) {
    if (width <= 0 || height <= 0) return 0;
    return depthLevelOffsetFloats(width, height, vqhip_mip_level_count(width, height)) * 4;
}

namespace {
// the hierarchy kernels over `src` (a plane, or the four samples per pixel) on `st`; arguments are validated by the callers
int enqueueDepthHierarchy(vqhip_ctx* ctx, hipStream_t st, const float* src, int srcPitch, int W, int H, float* mips, unsigned flags, bool ms) {
    HierArgs a;
    std::memset(&a, 0, sizeof(a));
    a.src = src; a.mips = mips; a.width = W; a.height = H; a.srcPitch = srcPitch; a.flags = (int)flags;
    a.levels = vqhip_mip_level_count(W, H);
    for (int l = 0; l < a.levels; ++l) a.off[l] = (uint32_t)depthLevelOffsetFloats(W, H, l);
    // TRUE_TOP on a frame of more than one 64 x 64 tile: the tiles' minima pass from the first kernel to the second through the context's buffer
    const bool shared = (flags & VQHIP_DEPTH_HIERARCHY_TRUE_TOP) && ((W + 63) / 64) * ((H + 63) / 64) > 1;
    if (shared) {
        if (!ctx->hier) HIP_TRY(ctx, hipMalloc(&ctx->hier, sizeof(float) * kMaxDepthTiles));
        if (!ctx->hierFree) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->hierFree, hipEventDisableTiming));
        if (ctx->hierUsed) HIP_TRY(ctx, hipStreamWaitEvent(st, ctx->hierFree, 0));
        a.tileMin = (float*)ctx->hier;
    }
    hipError_t e = launch_depth_hierarchy(st, a, ms);
    if (e != hipSuccess) return failHip(ctx, e, "depth_hierarchy launch");
    if (shared) { HIP_TRY(ctx, hipEventRecord(ctx->hierFree, st)); ctx->hierUsed = true; }
    return VQHIP_OK;
}
} // namespace

int vqhip_depth_hierarchy(vqhip_ctx* ctx, void* stream, const float* depth, int depth_pitch_px, int width, int height, float* mips, unsigned flags) {
    vqk::Range range_("DownsampleDepth");
    if (!ctx) return fail(nullptr, VQHIP_ERR_INVALID_ARG, "depth_hierarchy: ctx is NULL");
    CTX_GUARD(ctx, "depth_hierarchy");
    if (!depth || !mips) return fail(ctx, VQHIP_ERR_INVALID_ARG, "depth_hierarchy: NULL argument");
    if (width <= 0 || height <= 0) return fail(ctx, VQHIP_ERR_INVALID_ARG, "depth_hierarchy: bad dimensions");
    if (flags & ~VQHIP_DEPTH_HIERARCHY_TRUE_TOP) return fail(ctx, VQHIP_ERR_INVALID_ARG, "depth_hierarchy: unknown flag");
    if (width > VQHIP_DEPTH_HIERARCHY_MAX_DIM || height > VQHIP_DEPTH_HIERARCHY_MAX_DIM)
        return fail(ctx, VQHIP_ERR_UNSUPPORTED, "depth_hierarchy: frames above 4096 in either dimension are not supported (the reference's SPD instance covers 12 reductions)");
    const int pitch = depth_pitch_px ? depth_pitch_px : width;
    if (pitch < width) return fail(ctx, VQHIP_ERR_INVALID_ARG, "depth_hierarchy: pitch below the width");
    if (rangesOverlap(depth, ((size_t)(height - 1) * pitch + width) * 4, mips, vqhip_depth_hierarchy_bytes(width, height)))
        return fail(ctx, VQHIP_ERR_INVALID_ARG, "depth_hierarchy: mips overlaps depth");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return enqueueDepthHierarchy(ctx, (hipStream_t)stream, depth, pitch, width, height, mips, flags, false);
}

int vqhip_msaa_resolve_surfaces(vqhip_ctx* ctx, void* stream, const vqhip_msaa_surfaces* in,
        float* outDepth, int outDepthPitchPx, void* outNormals, vqhip_format outNormalsFmt, int outNormalsPitchPx,
        void* sceneColor, vqhip_format sceneFmt, int scenePitchPx, float* hierarchy, unsigned flags) {
    vqk::Range range_("MSAAResolve");
    const char* who = "msaa_resolve_surfaces";
    if (!ctx) return fail(nullptr, VQHIP_ERR_INVALID_ARG, "msaa_resolve_surfaces: ctx is NULL");
    CTX_GUARD(ctx, "msaa_resolve_surfaces");
    auto bad = [&](int code, const char* m) { return fail(ctx, code, std::string(who) + ": " + m); };
    if (!in) return bad(VQHIP_ERR_INVALID_ARG, "NULL argument");
    if (!outDepth && !outNormals && !sceneColor && !hierarchy) return bad(VQHIP_ERR_INVALID_ARG, "every output is NULL (the reference has no such permutation)");
    if (in->layers < 1 || in->layers > VQHIP_MSAA_MAX_LAYERS) return bad(VQHIP_ERR_INVALID_ARG, "layers must be 1..4");
    const int W = in->width, H = in->height;
    if (W <= 0 || H <= 0) return bad(VQHIP_ERR_INVALID_ARG, "bad dimensions");
    if (!in->depth_ms) return bad(VQHIP_ERR_INVALID_ARG, "depth_ms is NULL");
    if ((uintptr_t)in->depth_ms & 15u) return bad(VQHIP_ERR_INVALID_ARG, "depth_ms must be 16-byte aligned");
    if (flags & ~VQHIP_DEPTH_HIERARCHY_TRUE_TOP) return bad(VQHIP_ERR_INVALID_ARG, "unknown flag");
    auto pitchOf = [&](int p) { return p ? p : W; };
    const int depthPitch = pitchOf(in->depth_pitch_px), covPitch = pitchOf(in->coverage_pitch), bgPitch = pitchOf(in->background_pitch_px);
    const int odPitch = pitchOf(outDepthPitchPx), onPitch = pitchOf(outNormalsPitchPx), scPitch = pitchOf(scenePitchPx);
    if (depthPitch < W || (outDepth && odPitch < W) || (outNormals && onPitch < W) || (sceneColor && scPitch < W)) return bad(VQHIP_ERR_INVALID_ARG, "pitch below the width");
    const bool nIn32 = in->normals_fmt == VQHIP_FMT_RGBA32F, nOut32 = outNormalsFmt == VQHIP_FMT_RGBA32F;
    if (outNormals && ((!nIn32 && in->normals_fmt != VQHIP_FMT_R10G10B10A2_UNORM) || (!nOut32 && outNormalsFmt != VQHIP_FMT_R10G10B10A2_UNORM)))
        return bad(VQHIP_ERR_UNSUPPORTED, "normals must be R10G10B10A2_UNORM or RGBA32F");
    if (sceneColor && !isImageFmt(sceneFmt)) return bad(VQHIP_ERR_UNSUPPORTED, "sceneFmt must be RGBA32F or RGBA16F");
    if (hierarchy && (W > VQHIP_DEPTH_HIERARCHY_MAX_DIM || H > VQHIP_DEPTH_HIERARCHY_MAX_DIM))
        return bad(VQHIP_ERR_UNSUPPORTED, "hierarchy: frames above 4096 in either dimension are not supported");
    SurfArgs a;
    std::memset(&a, 0, sizeof(a));
    const size_t depthBytes = ((size_t)(H - 1) * depthPitch + W) * 16;
    const size_t nPx = nIn32 ? 16 : 4, scPx = sceneFmt == VQHIP_FMT_RGBA32F ? 16 : 8;
    struct Out { const void* p; size_t n; } outs[4] = {
        { outDepth, ((size_t)(H - 1) * odPitch + W) * 4 }, { outNormals, ((size_t)(H - 1) * onPitch + W) * (nOut32 ? 16 : 4) },
        { sceneColor, ((size_t)(H - 1) * scPitch + W) * scPx }, { hierarchy, vqhip_depth_hierarchy_bytes(W, H) } };
    auto aliases = [&](const void* p, size_t n) { for (const Out& o : outs) if (rangesOverlap(p, n, o.p, o.n)) return true; return false; };
    for (int i = 0; i < 4; ++i) for (int j = i + 1; j < 4; ++j)
        if (rangesOverlap(outs[i].p, outs[i].n, outs[j].p, outs[j].n)) return bad(VQHIP_ERR_INVALID_ARG, "outputs overlap each other");
    if (aliases(in->depth_ms, depthBytes)) return bad(VQHIP_ERR_INVALID_ARG, "an output overlaps depth_ms");
    if (outNormals || sceneColor) {
        if (covPitch < W) return bad(VQHIP_ERR_INVALID_ARG, "pitch below the width");
        for (int k = 0; k < in->layers; ++k) {
            if (!in->coverage[k]) return bad(VQHIP_ERR_INVALID_ARG, "NULL coverage plane");
            if (aliases(in->coverage[k], (size_t)(H - 1) * covPitch + W)) return bad(VQHIP_ERR_INVALID_ARG, "an output overlaps a coverage plane");
            a.L[k].cov = in->coverage[k];
            if (outNormals) {
                const int p = pitchOf(in->normals_pitch_px[k]);
                if (!in->normals[k]) return bad(VQHIP_ERR_INVALID_ARG, "NULL normals plane");
                if (p < W) return bad(VQHIP_ERR_INVALID_ARG, "pitch below the width");
                if (aliases(in->normals[k], ((size_t)(H - 1) * p + W) * nPx)) return bad(VQHIP_ERR_INVALID_ARG, "an output overlaps a normals plane");
                a.L[k].normals = in->normals[k]; a.L[k].nPitch = p;
            }
            if (sceneColor) {
                const int p = pitchOf(in->roughness_pitch_px[k]);
                if (!in->roughness[k]) return bad(VQHIP_ERR_INVALID_ARG, "NULL roughness (gb1) plane");
                if (p < W) return bad(VQHIP_ERR_INVALID_ARG, "pitch below the width");
                if (aliases(in->roughness[k], ((size_t)(H - 1) * p + W) * 16)) return bad(VQHIP_ERR_INVALID_ARG, "an output overlaps a roughness plane");
                a.L[k].gb1 = (const float4*)in->roughness[k]; a.L[k].rPitch = p;
            }
        }
        if (sceneColor && in->background) {
            if (bgPitch < W) return bad(VQHIP_ERR_INVALID_ARG, "pitch below the width");
            if (aliases(in->background, ((size_t)(H - 1) * bgPitch + W) * scPx)) return bad(VQHIP_ERR_INVALID_ARG, "an output overlaps the background");
            a.bg = in->background;
        }
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    a.depthMS = (const float4*)in->depth_ms;
    a.outDepth = outDepth; a.outNormals = outNormals; a.scene = sceneColor;
    a.width = W; a.height = H; a.layers = in->layers; a.covPitch = covPitch; a.depthPitch = depthPitch; a.bgPitch = bgPitch;
    a.outDepthPitch = odPitch; a.outNormalsPitch = onPitch; a.scenePitch = scPitch;
    a.nInF32 = nIn32; a.nOutF32 = nOut32; a.sceneF32 = sceneFmt == VQHIP_FMT_RGBA32F; a.arithDxc = ctx->arithDxc;
    if (hierarchy) {
        int rc = enqueueDepthHierarchy(ctx, st, in->depth_ms, depthPitch, W, H, hierarchy, flags, true);
        if (rc) return rc;
    }
    if (outDepth || outNormals || sceneColor) {
        hipError_t e = launch_resolve_surfaces(st, a);
        if (e != hipSuccess) return failHip(ctx, e, "msaa_resolve_surfaces launch");
    }
    return VQHIP_OK;
}

// ---- G-buffer producer --------------------------------------------------------------
size_t vqhip_mip_chain_bytes_rgba8(int w0, int h0, int nMips) { return vqhip_mip_level_offset_bytes(w0, h0, nMips) / 4; }

int vqhip_mip_chain_box_rgba8(vqhip_ctx* ctx, void* stream, void* mips, int w0, int h0, int nMips) {
    vqk::Range range_("GenerateMips");
    if (!ctx) return fail(nullptr, VQHIP_ERR_INVALID_ARG, "mip_chain_box_rgba8: ctx is NULL");
    CTX_GUARD(ctx, "mip_chain_box_rgba8");
    if (!mips || w0 <= 0 || h0 <= 0 || nMips <= 0 || nMips > vqhip_mip_level_count(w0, h0)) return fail(ctx, VQHIP_ERR_INVALID_ARG, "mip_chain_box_rgba8: bad argument");
    if ((w0 & (w0 - 1)) || (h0 & (h0 - 1))) return fail(ctx, VQHIP_ERR_UNSUPPORTED, "mip_chain_box_rgba8: w0 and h0 must be powers of two");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    for (int l = 1; l < nMips; ++l) {
        const void* src = (const char*)mips + vqhip_mip_level_offset_bytes(w0, h0, l - 1) / 4;
        void* dst = (char*)mips + vqhip_mip_level_offset_bytes(w0, h0, l) / 4;
        hipError_t e = launch_mip_box_rgba8((hipStream_t)stream, src, dst, mipDim(w0, l - 1), mipDim(h0, l - 1), mipDim(w0, l), mipDim(h0, l));
        if (e != hipSuccess) return failHip(ctx, e, "mip_box_rgba8 launch");
    }
    return VQHIP_OK;
}

int vqhip_max_materials(void) { return kMaxMaterials; }

static bool badTexture(const vqhip_texture2d& t) {
    return t.texels && (t.width <= 0 || t.height <= 0 || t.mips <= 0 || t.mips > vqhip_mip_level_count(t.width, t.height));
}

// The producers' kernels address a float4 plane with 32-bit byte offsets and pack pixel coordinates into 24 bits; `boundHeight`: the interpolant planes, whose
// height no earlier check has bounded
static int planeFitsOffsets(vqhip_ctx* ctx, const std::string& w, int pitch, int height, bool boundHeight = false) {
    if ((uint64_t)pitch * height * 16u >= (1ull << 32) || pitch >= (1 << 24) || (boundHeight && height >= (1 << 24)))
        return fail(ctx, VQHIP_ERR_UNSUPPORTED, w + ": a plane must be smaller than 4 GiB (32-bit offsets in the kernel)");
    return VQHIP_OK;
}
static int validateProducer(vqhip_ctx* ctx, const char* who, const vqhip_interpolants* in, const vqhip_material* materials, int numMaterials, const vqhip_ssao* ssao) {
    const std::string w(who);
    if (!in || !in->ip0 || !in->ip1 || !in->ip2) return fail(ctx, VQHIP_ERR_INVALID_ARG, w + ": NULL plane");
    if (in->width <= 0 || in->height <= 0 || in->row_pitch_px < in->width) return fail(ctx, VQHIP_ERR_INVALID_ARG, w + ": bad dimensions / pitch");
    if (const int rc = planeFitsOffsets(ctx, w, in->row_pitch_px, in->height, true)) return rc;
    if (numMaterials < 0 || numMaterials > kMaxMaterials || (numMaterials > 0 && !materials))
        return fail(ctx, VQHIP_ERR_INVALID_ARG, w + ": bad materials / numMaterials (see vqhip_max_materials)");
    for (int i = 0; i < numMaterials; ++i) {
        const vqhip_material& m = materials[i];
        if (badTexture(m.texDiffuse) || badTexture(m.texNormals) || badTexture(m.texEmissive) || badTexture(m.texMetalness) ||
            badTexture(m.texRoughness) || badTexture(m.texOcclRoughMetal) || badTexture(m.texLocalAO))
            return fail(ctx, VQHIP_ERR_INVALID_ARG, w + ": material " + std::to_string(i) + " has a texture with bad dimensions / mip count");
    }
    if (ssao && ssao->texels && (ssao->width <= 0 || ssao->height <= 0)) return fail(ctx, VQHIP_ERR_INVALID_ARG, w + ": bad ssao dimensions");
    return VQHIP_OK;
}
static size_t fillGbufConstants(vqhip_ctx* ctx, int slot, const vqhip_material* materials, int numMaterials, float ambient, const vqhip_ssao* ssao) {
    GbufConstants* gc = (GbufConstants*)(ctx->hostRing + (size_t)slot * kConstSlotBytes);
    std::memset(gc, 0, offsetof(GbufConstants, mats));
    gc->ambient = ambient;
    gc->numMaterials = numMaterials;
    gc->arithDxc = ctx->arithDxc;
    if (ssao && ssao->texels) gc->ssao = *ssao;
    if (numMaterials > 0) std::memcpy(gc->mats, materials, (size_t)numMaterials * sizeof(vqhip_material));
    return offsetof(GbufConstants, mats) + (size_t)numMaterials * sizeof(vqhip_material);
}

// The quad-uv plane of the _quad producers (docs/DESIGN_DETAILS.md §7.20 Q2), validated after validateProducer. `outs`: every plane the call writes (p NULL: a target that
// is not bound); the extent the kernel reads of quadUV must lie on none of them
static int validateQuadPlane(vqhip_ctx* ctx, const std::string& w, const vqhip_interpolants* in, const void* quadUV, int quad_pitch_px, const Span* outs, int nOut, QuadPlane* qp) {
    if (!quadUV) return fail(ctx, VQHIP_ERR_INVALID_ARG, w + ": quadUV is NULL");
    if ((uintptr_t)quadUV % 16) return fail(ctx, VQHIP_ERR_INVALID_ARG, w + ": quadUV is not 16-byte aligned");
    if (quad_pitch_px < 0) return fail(ctx, VQHIP_ERR_INVALID_ARG, w + ": negative quad_pitch_px");
    const int pitch = quad_pitch_px ? quad_pitch_px : in->row_pitch_px;
    if (pitch < in->width) return fail(ctx, VQHIP_ERR_INVALID_ARG, w + ": quad_pitch_px below the width");
    if (const int rc = planeFitsOffsets(ctx, w, pitch, in->height)) return rc;
    if (overlapsAny({ quadUV, planeExtent(in->width, in->height, pitch, 16), "" }, outs, nOut)) return fail(ctx, VQHIP_ERR_INVALID_ARG, w + ": quadUV overlaps an output");
    qp->uv = const_cast<void*>(quadUV); qp->pitch = (uint32_t)pitch;
    return VQHIP_OK;
}
// a plane of the draw's frame that the call writes, `bpp` bytes per pixel, as an entry of that list
static Span written(const vqhip_interpolants* in, const void* p, int pitch, size_t bpp) { return { p, planeExtent(in->width, in->height, pitch, bpp), "" }; }
// the interpolant planes and the frame as the producers' kernels take them; a->gc comes from stageConstants, the four G-buffer planes from gbufferPlanes (or stay NULL)
static void gbufArgs(GbufArgs* a, const vqhip_interpolants* in, int outPitch) {
    a->ip0 = (const float4*)in->ip0; a->ip1 = (const float4*)in->ip1; a->ip2 = (const float4*)in->ip2;
    a->width = in->width; a->height = in->height; a->pitch = in->row_pitch_px; a->outPitch = outPitch;
}

// vqhip_gbuffer_from_materials (quad == false) and its _quad form: one body, the launch differs
static int gbufferFromMaterials(vqhip_ctx* ctx, const std::string& w, bool quad, void* stream, const vqhip_interpolants* in, const vqhip_material* materials, int numMaterials,
                                float fAmbientLightingFactor, const vqhip_ssao* ssao, const vqhip_gbuffer* out, const void* quadUV, int quad_pitch_px) {
    vqk::Range range_("Geometry");                       // :1723 (surface assembly half of the lit draws)
    GbufArgs a;
    if (!out || !gbufferPlanes(*out, &a)) return fail(ctx, VQHIP_ERR_INVALID_ARG, w + ": NULL plane");
    int rc = validateProducer(ctx, w.c_str(), in, materials, numMaterials, ssao);
    if (rc) return rc;
    if (out->width != in->width || out->height != in->height || out->row_pitch_px < in->width)
        return fail(ctx, VQHIP_ERR_INVALID_ARG, w + ": bad dimensions / pitch");
    if ((rc = planeFitsOffsets(ctx, w, out->row_pitch_px, out->height)) != VQHIP_OK) return rc;
    QuadPlane qp = { nullptr, 0 };
    if (quad) {
        const Span outs[] = { written(in, out->gb0, out->row_pitch_px, 16), written(in, out->gb1, out->row_pitch_px, 16), written(in, out->gb2, out->row_pitch_px, 16),
                              written(in, out->gb3, out->row_pitch_px, 16), written(in, in->ip2, in->row_pitch_px, 16) };     // ip2.w receives the discard's -1
        if ((rc = validateQuadPlane(ctx, w, in, quadUV, quad_pitch_px, outs, 5, &qp)) != VQHIP_OK) return rc;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    int slot;
    if ((rc = stageConstants(ctx, st, &slot, &a.gc, fillGbufConstants, materials, numMaterials, fAmbientLightingFactor, ssao)) != VQHIP_OK) return rc;
    gbufArgs(&a, in, out->row_pitch_px);
    hipError_t e = quad ? launch_gbuffer_from_materials_quad(st, a, qp) : launch_gbuffer_from_materials(st, a);
    if (e != hipSuccess) return failHip(ctx, e, (w + " launch").c_str());
    return releaseSlot(ctx, slot, st);
}
int vqhip_gbuffer_from_materials(vqhip_ctx* ctx, void* stream, const vqhip_interpolants* in, const vqhip_material* materials, int numMaterials,
                                 float fAmbientLightingFactor, const vqhip_ssao* ssao, const vqhip_gbuffer* out) {
    if (!ctx) return fail(nullptr, VQHIP_ERR_INVALID_ARG, "gbuffer_from_materials: ctx is NULL");
    CTX_GUARD(ctx, "gbuffer_from_materials");
    return gbufferFromMaterials(ctx, "gbuffer_from_materials", false, stream, in, materials, numMaterials, fAmbientLightingFactor, ssao, out, nullptr, 0);
}
int vqhip_gbuffer_from_materials_quad(vqhip_ctx* ctx, void* stream, const vqhip_interpolants* in, const vqhip_material* materials, int numMaterials,
                                      float fAmbientLightingFactor, const vqhip_ssao* ssao, const vqhip_gbuffer* out, const void* quadUV, int quad_pitch_px) {
    if (!ctx) return fail(nullptr, VQHIP_ERR_INVALID_ARG, "gbuffer_from_materials_quad: ctx is NULL");
    CTX_GUARD(ctx, "gbuffer_from_materials_quad");
    return gbufferFromMaterials(ctx, "gbuffer_from_materials_quad", true, stream, in, materials, numMaterials, fAmbientLightingFactor, ssao, out, quadUV, quad_pitch_px);
}

// The colour target of the Z pre-pass (DepthPrePass.hlsl:PSMain :153-171; VQRenderer::RenderDepthPrePass, SceneRendering.cpp:1264-1360): Tex_SceneNormals.
static int sceneNormalsFromMaterials(vqhip_ctx* ctx, const std::string& w, bool quad, void* stream, const vqhip_interpolants* in, const vqhip_material* materials,
                                     int numMaterials, void* out, vqhip_format outFmt, int out_row_pitch_px, const void* quadUV, int quad_pitch_px) {
    vqk::Range range_("RenderDepthPrePass");             // SceneRendering.cpp:1273
    if (!out) return fail(ctx, VQHIP_ERR_INVALID_ARG, w + ": out is NULL");
    if (outFmt != VQHIP_FMT_R10G10B10A2_UNORM && outFmt != VQHIP_FMT_RGBA32F)
        return fail(ctx, VQHIP_ERR_UNSUPPORTED, w + ": outFmt must be R10G10B10A2_UNORM or RGBA32F");
    int rc = validateProducer(ctx, w.c_str(), in, materials, numMaterials, nullptr);
    if (rc) return rc;
    const int pitch = out_row_pitch_px ? out_row_pitch_px : in->width;
    if (pitch < in->width) return fail(ctx, VQHIP_ERR_INVALID_ARG, w + ": bad output pitch");
    QuadPlane qp = { nullptr, 0 };
    if (quad) {
        const Span outs[] = { written(in, out, pitch, outFmt == VQHIP_FMT_RGBA32F ? 16 : 4) };
        if ((rc = validateQuadPlane(ctx, w, in, quadUV, quad_pitch_px, outs, 1, &qp)) != VQHIP_OK) return rc;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    int slot;
    GbufArgs a = {};
    if ((rc = stageConstants(ctx, st, &slot, &a.gc, fillGbufConstants, materials, numMaterials, 0.0f, (const vqhip_ssao*)nullptr)) != VQHIP_OK) return rc;
    gbufArgs(&a, in, pitch);
    hipError_t e = quad ? launch_scene_normals_from_materials_quad(st, a, out, outFmt, qp) : launch_scene_normals_from_materials(st, a, out, outFmt);
    if (e != hipSuccess) return failHip(ctx, e, (w + " launch").c_str());
    return releaseSlot(ctx, slot, st);
}
int vqhip_scene_normals_from_materials(vqhip_ctx* ctx, void* stream, const vqhip_interpolants* in, const vqhip_material* materials, int numMaterials,
                                       void* out, vqhip_format outFmt, int out_row_pitch_px) {
    if (!ctx) return fail(nullptr, VQHIP_ERR_INVALID_ARG, "scene_normals_from_materials: ctx is NULL");
    CTX_GUARD(ctx, "scene_normals_from_materials");
    return sceneNormalsFromMaterials(ctx, "scene_normals_from_materials", false, stream, in, materials, numMaterials, out, outFmt, out_row_pitch_px, nullptr, 0);
}
int vqhip_scene_normals_from_materials_quad(vqhip_ctx* ctx, void* stream, const vqhip_interpolants* in, const vqhip_material* materials, int numMaterials,
                                            void* out, vqhip_format outFmt, int out_row_pitch_px, const void* quadUV, int quad_pitch_px) {
    if (!ctx) return fail(nullptr, VQHIP_ERR_INVALID_ARG, "scene_normals_from_materials_quad: ctx is NULL");
    CTX_GUARD(ctx, "scene_normals_from_materials_quad");
    return sceneNormalsFromMaterials(ctx, "scene_normals_from_materials_quad", true, stream, in, materials, numMaterials, out, outFmt, out_row_pitch_px, quadUV, quad_pitch_px);
}

// PSMain as the engine runs it (ForwardLighting.hlsl:226-380, the lit draws of RenderSceneColor, SceneRendering.cpp:1619-1760): interpolants +
// materials in, scene colour out, one kernel — the G-buffer record stays in registers. Two ring slots: the producer's constants and the lighting's.
static int forwardFromMaterials(vqhip_ctx* ctx, const std::string& w, bool quad, void* stream, const vqhip_interpolants* in, const vqhip_material* materials, int numMaterials,
        const vqhip_ssao* ssao, const VQ_PerFrameData* perFrame, const VQ_PerViewLightingData* perView,
        const VQ_PointLight* extraPoint, int numExtraPoint, const vqhip_envmap* env, const vqhip_shadowmaps* sm,
        void* out, int out_row_pitch_px, vqhip_format outFmt, const vqhip_psmain_targets* targets, const void* quadUV, int quad_pitch_px) {
    vqk::Range range_("RenderSceneColor");
    if (!out) return fail(ctx, VQHIP_ERR_INVALID_ARG, w + ": out is NULL");
    int rc = validateProducer(ctx, w.c_str(), in, materials, numMaterials, ssao);
    if (rc) return rc;
    if (out_row_pitch_px < in->width) return fail(ctx, VQHIP_ERR_INVALID_ARG, w + ": bad output pitch");
    bool casters = false;
    rc = validateLighting(ctx, w.c_str(), perFrame, perView, extraPoint, numExtraPoint, env, sm, outFmt, &casters);
    if (rc) return rc;
    MrtArgs mrt;
    if ((rc = fillMrt(ctx, w.c_str(), targets, in->width, &mrt)) != VQHIP_OK) return rc;
    QuadPlane qp = { nullptr, 0 };
    if (quad) {
        const Span outs[] = { written(in, out, out_row_pitch_px, outFmt == VQHIP_FMT_RGBA32F ? 16 : 8), written(in, in->ip2, in->row_pitch_px, 16),      // ip2.w receives the discard's -1
                              written(in, mrt.albedo, mrt.albedoPitch, mrt.albedoF32 ? 16 : 8), written(in, mrt.motion, mrt.motionPitch, mrt.motionF32 ? 8 : 4) };
        if ((rc = validateQuadPlane(ctx, w, in, quadUV, quad_pitch_px, outs, 4, &qp)) != VQHIP_OK) return rc;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    int slotG, slotF;
    GbufArgs a = {};
    const FrameConstants* fc;
    if ((rc = stageConstants(ctx, st, &slotG, &a.gc, fillGbufConstants, materials, numMaterials, perFrame->fAmbientLightingFactor, ssao)) != VQHIP_OK ||     // cbPerFrame.fAmbientLightingFactor, :247
        (rc = stageConstants(ctx, st, &slotF, &fc, fillFrameConstants, perFrame, perView, extraPoint, numExtraPoint, env, sm)) != VQHIP_OK) return rc;
    gbufArgs(&a, in, 0);
    hipError_t e = quad ? launch_forward_from_materials_quad(st, a, fc, env != nullptr, casters, out, out_row_pitch_px, outFmt, ctx->arithDxc, ctx->opt, mrt, qp)
                        : launch_forward_from_materials(st, a, fc, env != nullptr, casters, out, out_row_pitch_px, outFmt, ctx->arithDxc, ctx->opt, mrt);
    if (e != hipSuccess) return failHip(ctx, e, (w + " launch").c_str());
    if ((rc = releaseSlot(ctx, slotG, st)) != VQHIP_OK) return rc;
    return releaseSlot(ctx, slotF, st);
}
int vqhip_forward_lighting_from_materials(vqhip_ctx* ctx, void* stream, const vqhip_interpolants* in, const vqhip_material* materials, int numMaterials,
        const vqhip_ssao* ssao, const VQ_PerFrameData* perFrame, const VQ_PerViewLightingData* perView,
        const VQ_PointLight* extraPoint, int numExtraPoint, const vqhip_envmap* env, const vqhip_shadowmaps* sm,
        void* out, int out_row_pitch_px, vqhip_format outFmt) {
    if (!ctx) return fail(nullptr, VQHIP_ERR_INVALID_ARG, "forward_lighting_from_materials: ctx is NULL");
    CTX_GUARD(ctx, "forward_lighting_from_materials");
    return forwardFromMaterials(ctx, "forward_lighting_from_materials", false, stream, in, materials, numMaterials, ssao, perFrame, perView, extraPoint, numExtraPoint, env, sm,
                                out, out_row_pitch_px, outFmt, nullptr, nullptr, 0);
}
int vqhip_forward_lighting_from_materials_mrt(vqhip_ctx* ctx, void* stream, const vqhip_interpolants* in, const vqhip_material* materials, int numMaterials,
        const vqhip_ssao* ssao, const VQ_PerFrameData* perFrame, const VQ_PerViewLightingData* perView,
        const VQ_PointLight* extraPoint, int numExtraPoint, const vqhip_envmap* env, const vqhip_shadowmaps* sm,
        void* out, int out_row_pitch_px, vqhip_format outFmt, const vqhip_psmain_targets* targets) {
    if (!ctx) return fail(nullptr, VQHIP_ERR_INVALID_ARG, "forward_lighting_from_materials: ctx is NULL");
    CTX_GUARD(ctx, "forward_lighting_from_materials");
    return forwardFromMaterials(ctx, "forward_lighting_from_materials", false, stream, in, materials, numMaterials, ssao, perFrame, perView, extraPoint, numExtraPoint, env, sm,
                                out, out_row_pitch_px, outFmt, targets, nullptr, 0);
}
int vqhip_forward_lighting_from_materials_quad(vqhip_ctx* ctx, void* stream, const vqhip_interpolants* in, const vqhip_material* materials, int numMaterials,
        const vqhip_ssao* ssao, const VQ_PerFrameData* perFrame, const VQ_PerViewLightingData* perView,
        const VQ_PointLight* extraPoint, int numExtraPoint, const vqhip_envmap* env, const vqhip_shadowmaps* sm,
        void* out, int out_row_pitch_px, vqhip_format outFmt, const vqhip_psmain_targets* targets, const void* quadUV, int quad_pitch_px) {
    if (!ctx) return fail(nullptr, VQHIP_ERR_INVALID_ARG, "forward_lighting_from_materials_quad: ctx is NULL");
    CTX_GUARD(ctx, "forward_lighting_from_materials_quad");
    return forwardFromMaterials(ctx, "forward_lighting_from_materials_quad", true, stream, in, materials, numMaterials, ssao, perFrame, perView, extraPoint, numExtraPoint, env, sm,
                                out, out_row_pitch_px, outFmt, targets, quadUV, quad_pitch_px);
}

// ---- skydome ------------------------------------------------------------------------
int vqhip_skydome(vqhip_ctx* ctx, void* stream, const void* equirect_level0, int w0, int h0, const VQ_SkydomeParams* params,
                  const vqhip_interpolants* coverage, void* color, int width, int height, int row_pitch_px, vqhip_format fmt) {
    vqk::Range range_("EnvironmentMap");                 // SceneRendering.cpp:1824
    if (!ctx) return fail(nullptr, VQHIP_ERR_INVALID_ARG, "skydome: ctx is NULL");
    CTX_GUARD(ctx, "skydome");
    if (!equirect_level0 || !params || !color || w0 <= 0 || h0 <= 0 || width <= 0 || height <= 0 || row_pitch_px < width)
        return fail(ctx, VQHIP_ERR_INVALID_ARG, "skydome: bad argument");
    if (!isImageFmt(fmt)) return fail(ctx, VQHIP_ERR_UNSUPPORTED, "skydome: fmt must be RGBA32F or RGBA16F");
    if (coverage && (!coverage->ip2 || coverage->width != width || coverage->height != height || coverage->row_pitch_px < width))
        return fail(ctx, VQHIP_ERR_INVALID_ARG, "skydome: coverage planes do not match the colour target");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipError_t e = launch_skydome((hipStream_t)stream, (const float4*)equirect_level0, w0, h0, *params,
                                  coverage ? (const float4*)coverage->ip2 : nullptr, coverage ? coverage->row_pitch_px : 0,
                                  color, width, height, row_pitch_px, fmt);
    return e == hipSuccess ? VQHIP_OK : failHip(ctx, e, "skydome launch");
}

int vqhip_unlit_composite(vqhip_ctx* ctx, void* stream, const vqhip_interpolants* coverage, const VQ_float4* colors, int numColors,
                          void* color, int width, int height, int row_pitch_px, vqhip_format fmt) {
    vqk::Range range_("Lights");                         // :1790
    if (!ctx) return fail(nullptr, VQHIP_ERR_INVALID_ARG, "unlit_composite: ctx is NULL");
    CTX_GUARD(ctx, "unlit_composite");
    if (!coverage || !coverage->ip2 || !color || width <= 0 || height <= 0 || row_pitch_px < width || numColors < 0 || (numColors > 0 && !colors))
        return fail(ctx, VQHIP_ERR_INVALID_ARG, "unlit_composite: bad argument");
    if (numColors > VQHIP_MAX_UNLIT_COLORS) return fail(ctx, VQHIP_ERR_INVALID_ARG, "unlit_composite: more than VQHIP_MAX_UNLIT_COLORS gizmos");
    if (coverage->width != width || coverage->height != height || coverage->row_pitch_px < width)
        return fail(ctx, VQHIP_ERR_INVALID_ARG, "unlit_composite: coverage planes do not match the colour target");
    if (!isImageFmt(fmt)) return fail(ctx, VQHIP_ERR_UNSUPPORTED, "unlit_composite: fmt must be RGBA32F or RGBA16F");
    if (numColors == 0) return VQHIP_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    UnlitColors cols;
    for (int i = 0; i < numColors; ++i) cols.c[i] = make_float4(colors[i].x, colors[i].y, colors[i].z, colors[i].w);
    hipError_t e = launch_unlit_composite((hipStream_t)stream, (const float4*)coverage->ip2, coverage->row_pitch_px, cols, numColors,
                                          color, width, height, row_pitch_px, fmt);
    return e == hipSuccess ? VQHIP_OK : failHip(ctx, e, "unlit_composite launch");
}

// ---- HDRI ingest --------------------------------------------------------------------
int vqhip_hdr_parse_header(const void* file, size_t bytes, int* width, int* height, size_t* data_offset) {
    if (!file || !width || !height) return fail(nullptr, VQHIP_ERR_INVALID_ARG, "hdr_parse_header: NULL argument");
    const char* err = nullptr; size_t off = 0;
    if (hdr_parse_header((const uint8_t*)file, bytes, width, height, &off, &err)) return fail(nullptr, VQHIP_ERR_INVALID_ARG, err);
    if (data_offset) *data_offset = off;
    return VQHIP_OK;
}

int vqhip_hdr_decode_rgba32f(vqhip_ctx* ctx, void* stream, const void* file, size_t bytes, void* out_rgba32f, int width, int height) {
    vqk::Range range_("LoadHDRI");
    if (!ctx) return fail(nullptr, VQHIP_ERR_INVALID_ARG, "hdr_decode: ctx is NULL");
    CTX_GUARD(ctx, "hdr_decode");
    if (!file || !out_rgba32f) return fail(ctx, VQHIP_ERR_INVALID_ARG, "hdr_decode: NULL argument");
    const char* err = nullptr; int w = 0, h = 0; size_t off = 0;
    if (hdr_parse_header((const uint8_t*)file, bytes, &w, &h, &off, &err)) return fail(ctx, VQHIP_ERR_INVALID_ARG, err);
    if (w != width || h != height) return fail(ctx, VQHIP_ERR_INVALID_ARG, "hdr_decode: width/height do not match the file header");
    const size_t px = (size_t)w * h;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    // run-length coded files: the host walks the run headers (offsets of every byte plane, validation), the GPU expands the runs and converts (hdri.hip:k_hdr_expand)
    {
        std::vector<uint32_t> planeOff(4 * (size_t)h + 1);
        const int wr = hdr_walk_runs((const uint8_t*)file, bytes, off, w, h, planeOff.data(), &err);
        if (wr < 0) return fail(ctx, VQHIP_ERR_INVALID_ARG, err);
        int encCap = 0, pitch = 0, ldsBytes = 0;
        if (wr == 0 && hdr_expand_fits(planeOff.data(), w, h, ctx->ldsPerBlock, &encCap, &pitch, &ldsBytes)) {
            const size_t used = planeOff[4 * (size_t)h], fileDev = (used + 4 + 255) & ~(size_t)255, tabBytes = planeOff.size() * 4;
            const int rc = ensureScratch(ctx, fileDev + tabBytes);
            if (rc) return rc;
            // the offset table is a pageable host vector: whatever happens below, the stream is drained before this scope (and the vector) ends
            hipError_t e = hipMemcpyAsync(ctx->scratch, file, used, hipMemcpyHostToDevice, st);
            if (e == hipSuccess) e = hipMemcpyAsync((char*)ctx->scratch + fileDev, planeOff.data(), tabBytes, hipMemcpyHostToDevice, st);
            const bool copied = e == hipSuccess;
            if (copied) e = launch_hdr_expand(st, ctx->scratch, (char*)ctx->scratch + fileDev, out_rgba32f, w, h, encCap, pitch, ldsBytes);
            const hipError_t es = hipStreamSynchronize(st);  // load-time call: the offset table and the scratch buffer are free again on return
            if (!copied) return failHip(ctx, e, "hdr_decode upload");
            if (e == hipSuccess && es == hipSuccess) return VQHIP_OK;
            if (es != hipSuccess) return failHip(ctx, es, "hdr_expand");
            (void)hipGetLastError();                         // the launch was refused (e.g. the LDS opt-in on a part with less LDS): the host expansion below still decodes the file
        }
    }
    // flat files, scanlines too wide for the LDS: expansion on the host, conversion on the GPU
    std::vector<uint8_t> rgbe(px * 4);
    if (hdr_expand_rgbe((const uint8_t*)file, bytes, off, w, h, rgbe.data(), &err)) return fail(ctx, VQHIP_ERR_INVALID_ARG, err);
    int rc = ensureScratch(ctx, px * 4);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->scratch, rgbe.data(), px * 4, hipMemcpyHostToDevice, st));
    hipError_t e = launch_rgbe_to_rgba32f(st, ctx->scratch, out_rgba32f, px);
    if (e != hipSuccess) return failHip(ctx, e, "rgbe_to_rgba32f launch");
    HIP_TRY(ctx, hipStreamSynchronize(st));      // load-time call: the staging vector and the scratch buffer are free again on return
    return VQHIP_OK;
}

// ---- FSR 1.0 ------------------------------------------------------------------------
static uint32_t fbits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

// FsrEasuCon, ffx_fsr1.h:156-203, as called on the CPU by FFSR1_EASU::UpdateEASUConstantBlock (PostProcess.cpp:47-79)
int vqhip_hdr_downsize_rgba32f(vqhip_ctx* ctx, void* stream, const void* in, int width, int height, void* out, int out_width, int out_height) {
    vqk::Range range_("DownsizeHDRI");
    if (!ctx) return fail(nullptr, VQHIP_ERR_INVALID_ARG, "hdr_downsize: ctx is NULL");
    CTX_GUARD(ctx, "hdr_downsize");
    if (!in || !out || width <= 0 || height <= 0 || out_width <= 0 || out_height <= 0) return fail(ctx, VQHIP_ERR_INVALID_ARG, "hdr_downsize: bad argument");
    if (in == out) return fail(ctx, VQHIP_ERR_INVALID_ARG, "hdr_downsize: in-place is not supported");
    const int k = width / out_width;
    if (k < 1 || out_width * k != width || out_height * k != height)
        return fail(ctx, VQHIP_ERR_UNSUPPORTED, "hdr_downsize: only integer ratios, the same in x and y, are implemented (the engine's 8k/4k/2k/1k table); "
                                                "general resampling (stb_image_resize, absent from the reference tree) is not");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (k == 1) { HIP_TRY(ctx, hipMemcpyAsync(out, in, (size_t)width * height * 16, hipMemcpyDeviceToDevice, (hipStream_t)stream)); return VQHIP_OK; }
    hipError_t e = launch_downsize_box((hipStream_t)stream, in, out, width, height, k);
    return e == hipSuccess ? VQHIP_OK : failHip(ctx, e, "downsize launch");
}

void vqhip_fsr_easu_con(uint32_t con[16], float inVpW, float inVpH, float inSzW, float inSzH, float outW, float outH) {
    const float rOutW = 1.0f / outW, rOutH = 1.0f / outH, rInW = 1.0f / inSzW, rInH = 1.0f / inSzH;
    con[0] = fbits(inVpW * rOutW);                 con[1] = fbits(inVpH * rOutH);
    con[2] = fbits(0.5f * inVpW * rOutW - 0.5f);   con[3] = fbits(0.5f * inVpH * rOutH - 0.5f);
    con[4] = fbits(rInW);                          con[5] = fbits(rInH);
    con[6] = fbits(1.0f * rInW);                   con[7] = fbits(-1.0f * rInH);
    con[8] = fbits(-1.0f * rInW);                  con[9] = fbits(2.0f * rInH);
    con[10] = fbits(1.0f * rInW);                  con[11] = fbits(2.0f * rInH);
    con[12] = fbits(0.0f * rInW);                  con[13] = fbits(4.0f * rInH);
    con[14] = con[15] = 0;
}
// FsrRcasCon, ffx_fsr1.h:662-674 (FFSR1_RCAS::UpdateRCASConstantBlock, PostProcess.cpp:39-45)
void vqhip_fsr_rcas_con(uint32_t con[4], float sharpnessStops) {
    const float s = exp2f(-sharpnessStops);
    // ffx_a.h:482-550 packs the CPU-side half by TRUNCATION (table lookup on sign+exponent, mantissa shifted right), flushing
    // sub-denormals to zero and saturating overflow / inf / NaN to 65504 — not round-to-nearest: 0.2 stops gives 0x3af6, not 0x3af7
    const uint32_t u = fbits(s), sg = (u >> 16) & 0x8000u, e = (u >> 23) & 0xffu, m = u & 0x7fffffu;
    const uint32_t hb = e < 103 ? sg : e < 113 ? sg + (1u << (e - 103)) + (m >> (126 - e)) : e < 143 ? sg + ((e - 112) << 10) + (m >> 13) : sg + 0x7bffu;
    con[0] = fbits(s); con[1] = hb | (hb << 16); con[2] = 0; con[3] = 0;
}

static bool isColorFmt(int f) { return f == VQHIP_FMT_RGBA32F || f == VQHIP_FMT_RGBA16F || f == VQHIP_FMT_RGBA8_UNORM; }

int vqhip_fsr_easu(vqhip_ctx* ctx, void* stream, const void* in, int inW, int inH, vqhip_format inFmt, const uint32_t con[16],
                   void* out, int outW, int outH, vqhip_format outFmt) {
    vqk::Range range_("FSR-EASU CS");
    if (!ctx) return fail(nullptr, VQHIP_ERR_INVALID_ARG, "fsr_easu: ctx is NULL");
    CTX_GUARD(ctx, "fsr_easu");
    if (!in || !out || !con || inW <= 0 || inH <= 0 || outW <= 0 || outH <= 0 || inW >= (1 << 24) || outW >= (1 << 24))
        return fail(ctx, VQHIP_ERR_INVALID_ARG, "fsr_easu: bad argument");
    if (!isColorFmt(inFmt) || !isColorFmt(outFmt)) return fail(ctx, VQHIP_ERR_UNSUPPORTED, "fsr_easu: formats must be RGBA8_UNORM, RGBA16F or RGBA32F");
    if (in == out) return fail(ctx, VQHIP_ERR_INVALID_ARG, "fsr_easu: in-place is not supported");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipError_t e = launch_fsr_easu((hipStream_t)stream, in, inW, inH, inFmt, con, out, outW, outH, outFmt);
    return e == hipSuccess ? VQHIP_OK : failHip(ctx, e, "fsr_easu launch");
}

int vqhip_fsr_rcas(vqhip_ctx* ctx, void* stream, const void* in, void* out, int width, int height, const uint32_t con[4],
                   vqhip_format inFmt, vqhip_format outFmt) {
    vqk::Range range_("FSR-RCAS CS");
    if (!ctx) return fail(nullptr, VQHIP_ERR_INVALID_ARG, "fsr_rcas: ctx is NULL");
    CTX_GUARD(ctx, "fsr_rcas");
    if (!in || !out || !con || width <= 0 || height <= 0 || width >= (1 << 24)) return fail(ctx, VQHIP_ERR_INVALID_ARG, "fsr_rcas: bad argument");
    if (!isColorFmt(inFmt) || !isColorFmt(outFmt)) return fail(ctx, VQHIP_ERR_UNSUPPORTED, "fsr_rcas: formats must be RGBA8_UNORM, RGBA16F or RGBA32F");
    if (in == out) return fail(ctx, VQHIP_ERR_INVALID_ARG, "fsr_rcas: in-place is not supported");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipError_t e = launch_fsr_rcas((hipStream_t)stream, in, out, width, height, con, inFmt, outFmt);
    return e == hipSuccess ? VQHIP_OK : failHip(ctx, e, "fsr_rcas launch");
}

int vqhip_visualize(vqhip_ctx* ctx, void* stream, const void* in, void* out, int width, int height, const VQ_VizParams* params,
                    vqhip_format inFmt, vqhip_format outFmt) {
    vqk::Range range_("RenderPostProcess_DebugViz");      // :2543
    if (!ctx) return fail(nullptr, VQHIP_ERR_INVALID_ARG, "visualize: ctx is NULL");
    CTX_GUARD(ctx, "visualize");
    if (!in || !out || !params || width <= 0 || height <= 0 || (uint64_t)width * height >= (1ull << 28)) return fail(ctx, VQHIP_ERR_INVALID_ARG, "visualize: bad argument");
    // inputs: whatever the draw mode's SRV holds (SceneRendering.cpp:2555-2566) — colour formats, Tex_SceneNormals (R10G10B10A2), Tex_SceneMotionVectors (RG16F | RG32F)
    const bool inOk = isColorFmt(inFmt) || inFmt == VQHIP_FMT_R10G10B10A2_UNORM || inFmt == VQHIP_FMT_RG16F || inFmt == VQHIP_FMT_RG32F;
    if (!inOk || !isColorFmt(outFmt)) return fail(ctx, VQHIP_ERR_UNSUPPORTED, "visualize: inFmt must be RGBA8_UNORM, RGBA16F, RGBA32F, RG16F, RG32F or R10G10B10A2_UNORM; outFmt RGBA8_UNORM, RGBA16F or RGBA32F");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipError_t e = launch_visualize((hipStream_t)stream, in, out, width, height, *params, inFmt, outFmt);
    return e == hipSuccess ? VQHIP_OK : failHip(ctx, e, "visualize launch");
}

int vqhip_apply_reflections(vqhip_ctx* ctx, void* stream, const void* reflectionRadiance, void* sceneColor, int width, int height, vqhip_format fmt) {
    if (!ctx) return fail(nullptr, VQHIP_ERR_INVALID_ARG, "apply_reflections: ctx is NULL");
    CTX_GUARD(ctx, "apply_reflections");
    return vqhip_composite_reflections(ctx, stream, reflectionRadiance, nullptr, sceneColor, width, height, fmt);
}

// VQRenderer::CompositeReflections (SceneRendering.cpp:2362-2403): ApplyReflectionsPass in the permutation its SRVBoundingVolumes selects (ApplyReflections.cpp:62-68)
int vqhip_composite_reflections(vqhip_ctx* ctx, void* stream, const void* reflectionRadiance, const void* boundingVolumes, void* sceneColor, int width, int height, vqhip_format fmt) {
    vqk::Range range_("CompositeReflections");            // :2374
    if (!ctx) return fail(nullptr, VQHIP_ERR_INVALID_ARG, "composite_reflections: ctx is NULL");
    CTX_GUARD(ctx, "composite_reflections");
    if (!reflectionRadiance || !sceneColor || width <= 0 || height <= 0 || (uint64_t)width * height >= (1ull << 28)) return fail(ctx, VQHIP_ERR_INVALID_ARG, "composite_reflections: bad argument");
    if (!isImageFmt(fmt)) return fail(ctx, VQHIP_ERR_UNSUPPORTED, "composite_reflections: fmt must be RGBA32F or RGBA16F");
    if (boundingVolumes == sceneColor || reflectionRadiance == sceneColor) return fail(ctx, VQHIP_ERR_INVALID_ARG, "composite_reflections: the inputs must not alias the scene colour");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipError_t e = launch_apply_reflections((hipStream_t)stream, reflectionRadiance, boundingVolumes, sceneColor, width, height, fmt);
    return e == hipSuccess ? VQHIP_OK : failHip(ctx, e, "composite_reflections launch");
}

// ---- SSR front ends (docs/DESIGN_DETAILS.md §7.11-7.13): what the six entry points below share ----------------------------------------------------------------
namespace {
struct Plane { const void* p; int pitchPx; size_t bpp; const char* name; };           // one full-frame plane; pitchPx 0: dense rows
int pitchOr(int pitchPx, int W) { return pitchPx ? pitchPx : W; }
Span spanOf(int W, int H, const Plane& q) { return { q.p, planeExtent(W, H, pitchOr(q.pitchPx, W), q.bpp), q.name }; }
bool isNormalFmt(int f) { return f == VQHIP_FMT_R10G10B10A2_UNORM || f == VQHIP_FMT_RGBA32F; }
bool isAvgFmt(int f) { return f == VQHIP_FMT_R11G11B10_FLOAT || f == VQHIP_FMT_RGBA32F; }
size_t imgBpp(int f) { return f == VQHIP_FMT_RGBA32F ? 16 : 8; }
size_t nrmBpp(int f) { return f == VQHIP_FMT_RGBA32F ? 16 : 4; }
size_t avgBpp(int f) { return f == VQHIP_FMT_RGBA32F ? 16 : 4; }
size_t motionBpp(int f) { return f == VQHIP_FMT_RG32F ? 8 : 4; }
bool badEnv(const vqhip_envmap* env) { return !env->specular_cube || !env->brdf_lut || env->spec_res0 <= 0 || env->spec_mips <= 0 || env->lut_size <= 0; }
void copyEnvRotation(float (&rot)[3][3], const VQ_SSSRConstants* cb) { for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) rot[i][j] = cb->envMapRotation.m[i][j]; }
// cb->bufferDimensions as the frame; `suffix` ends the 4096 message. Returns VQHIP_OK or the failure already recorded in ctx
int ssrFrame(vqhip_ctx* ctx, const char* who, const VQ_SSSRConstants* cb, const char* suffix, int* W, int* H) {
    const uint32_t w = cb->bufferDimensions[0], h = cb->bufferDimensions[1];
    if (w == 0 || h == 0) return fail(ctx, VQHIP_ERR_INVALID_ARG, std::string(who) + ": bad bufferDimensions");
    if (w > VQHIP_DEPTH_HIERARCHY_MAX_DIM || h > VQHIP_DEPTH_HIERARCHY_MAX_DIM)
        return fail(ctx, VQHIP_ERR_UNSUPPORTED, std::string(who) + ": frames above 4096 in either dimension are not supported" + suffix);
    *W = (int)w; *H = (int)h;
    return VQHIP_OK;
}
const Plane* shortPitch(int W, const Plane* q, int n) {                                // the first plane whose rows are shorter than the frame's
    for (int i = 0; i < n; ++i) if (pitchOr(q[i].pitchPx, W) < W) return &q[i];
    return nullptr;
}
// The overlap questions of the denoiser passes beyond overlapsAny and overlapEachOther: outputs against the inputs, against the tile list. Each finds the pair; the caller words the refusal
const Plane* inputUnder(int W, int H, const Plane* in, int nIn, const Span* outs, int nOut) {     // the first input that one of `outs` lies on
    for (int i = 0; i < nIn; ++i) if (overlapsAny(spanOf(W, H, in[i]), outs, nOut)) return &in[i];
    return nullptr;
}
bool tilesUnder(int W, int H, const uint32_t* tileList, const uint32_t* counters, const Span* outs, int nOut) {
    return overlapsAny({ tileList, (size_t)((W + 7) / 8) * ((H + 7) / 8) * 4, "" }, outs, nOut) || overlapsAny({ counters, 8, "" }, outs, nOut);
}
} // namespace

int vqhip_ssr_environment_fallback(vqhip_ctx* ctx, void* stream, const void* sceneColorRoughness, vqhip_format sceneFmt, int scenePitchPx,
                                   const float* depth, int depthPitchPx, const void* normals, vqhip_format normalFmt, int normalPitchPx,
                                   int width, int height, const VQ_SSSRConstants* cb, const vqhip_envmap* env,
                                   void* outRadiance, vqhip_format outFmt, int outPitchPx, uint8_t* outExtractedRoughness) {
    vqk::Range range_("FFX DNSR ClassifyTiles");
    if (!ctx) return fail(nullptr, VQHIP_ERR_INVALID_ARG, "ssr_environment_fallback: ctx is NULL");
    CTX_GUARD(ctx, "ssr_environment_fallback");
    if (!sceneColorRoughness || !depth || !normals || !cb || !env || !outRadiance || width <= 0 || height <= 0 || (uint64_t)width * height >= (1ull << 28))
        return fail(ctx, VQHIP_ERR_INVALID_ARG, "ssr_environment_fallback: bad argument");
    if (!isImageFmt(sceneFmt) || !isImageFmt(outFmt)) return fail(ctx, VQHIP_ERR_UNSUPPORTED, "ssr_environment_fallback: scene colour and radiance must be RGBA32F or RGBA16F");
    if (!isNormalFmt(normalFmt)) return fail(ctx, VQHIP_ERR_UNSUPPORTED, "ssr_environment_fallback: normals must be R10G10B10A2_UNORM or RGBA32F");
    if (badEnv(env)) return fail(ctx, VQHIP_ERR_INVALID_ARG, "ssr_environment_fallback: env needs the specular cube and the BRDF LUT");
    const uint32_t mc = cb->envMapSpecularIrradianceCubemapMipLevelCount;
    if (mc < 1 || mc > (uint32_t)env->spec_mips) return fail(ctx, VQHIP_ERR_INVALID_ARG, "ssr_environment_fallback: envMapSpecularIrradianceCubemapMipLevelCount must be in [1, env->spec_mips]");
    SsrArgs a;
    a.scenePitch = pitchOr(scenePitchPx, width); a.depthPitch = pitchOr(depthPitchPx, width); a.normalPitch = pitchOr(normalPitchPx, width); a.outPitch = pitchOr(outPitchPx, width);
    if (a.scenePitch < width || a.depthPitch < width || a.normalPitch < width || a.outPitch < width) return fail(ctx, VQHIP_ERR_INVALID_ARG, "ssr_environment_fallback: pitch < width");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    a.scene = sceneColorRoughness; a.depth = depth; a.normals = normals; a.out = outRadiance; a.outRoughness = outExtractedRoughness;
    a.width = width; a.height = height;
    a.invProj = cb->invProjection; a.view = cb->view; a.invView = cb->invView;
    copyEnvRotation(a.rot, cb);
    a.invDimX = cb->inverseBufferDimensions[0]; a.invDimY = cb->inverseBufferDimensions[1];
    a.roughnessThreshold = cb->roughnessThreshold; a.mipCount = (float)mc;
    a.pow5ExpLog = ctx->pow5ExpLog; a.arithDxc = ctx->arithDxc; a.env = *env;
    hipError_t e = launch_ssr_env_fallback((hipStream_t)stream, a, sceneFmt, normalFmt, outFmt);
    return e == hipSuccess ? VQHIP_OK : failHip(ctx, e, "ssr_environment_fallback launch");
}

// ---- SSR ray list + hierarchical march (ssr_trace.hip; docs/DESIGN_DETAILS.md §7.11) ------------------------------------------------------
int vqhip_ssr_classify(vqhip_ctx* ctx, void* stream, const void* sceneColorRoughness, vqhip_format sceneFmt, int scenePitchPx,
                       const float* depth, int depthPitchPx, const void* varianceHistory, int variancePitchPx, const VQ_SSSRConstants* cb,
                       uint32_t* rayList, uint32_t* counters, uint32_t* denoiserTileList) {
    vqk::Range range_("FFX DNSR ClassifyTiles");
    if (!ctx) return fail(nullptr, VQHIP_ERR_INVALID_ARG, "ssr_classify: ctx is NULL");
    CTX_GUARD(ctx, "ssr_classify");
    if (!sceneColorRoughness || !depth || !cb || !rayList || !counters) return fail(ctx, VQHIP_ERR_INVALID_ARG, "ssr_classify: NULL argument");
    int W, H;
    if (int rc = ssrFrame(ctx, "ssr_classify", cb, " (the range of the depth hierarchy)", &W, &H)) return rc;
    if (!isImageFmt(sceneFmt)) return fail(ctx, VQHIP_ERR_UNSUPPORTED, "ssr_classify: the scene colour must be RGBA32F or RGBA16F");
    const int scenePitch = pitchOr(scenePitchPx, W), depthPitch = pitchOr(depthPitchPx, W), variancePitch = pitchOr(variancePitchPx, W);
    if (scenePitch < W || depthPitch < W || variancePitch < W) return fail(ctx, VQHIP_ERR_INVALID_ARG, "ssr_classify: pitch < width");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    if (!ctx->ssrTiles) HIP_TRY(ctx, hipMalloc(&ctx->ssrTiles, sizeof(uint32_t) * 2 * kMaxSsrTiles));
    if (!ctx->ssrFree) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ssrFree, hipEventDisableTiming));
    if (ctx->ssrUsed) HIP_TRY(ctx, hipStreamWaitEvent(st, ctx->ssrFree, 0));
    SsrClassifyArgs a;
    std::memset(&a, 0, sizeof(a));
    a.scene = sceneColorRoughness; a.depth = depth; a.variance = varianceHistory;
    a.rayList = rayList; a.counters = counters; a.tileList = denoiserTileList;
    a.tileRays = (uint32_t*)ctx->ssrTiles; a.tileFlag = a.tileRays + kMaxSsrTiles;
    a.width = W; a.height = H; a.scenePitch = scenePitch; a.depthPitch = depthPitch; a.variancePitch = variancePitch;
    a.sceneF32 = sceneFmt == VQHIP_FMT_RGBA32F;
    a.tilesX = (W + 7) / 8; a.tilesY = (H + 7) / 8;
    a.roughnessThreshold = cb->roughnessThreshold; a.varianceThreshold = cb->varianceThreshold;
    a.samplesPerQuad = cb->samplesPerQuad; a.varianceGuided = cb->temporalVarianceGuidedTracingEnabled;
    hipError_t e = launch_ssr_classify(st, a);
    if (e != hipSuccess) return failHip(ctx, e, "ssr_classify launch");
    HIP_TRY(ctx, hipEventRecord(ctx->ssrFree, st));
    ctx->ssrUsed = true;
    return VQHIP_OK;
}

int vqhip_ssr_intersect(vqhip_ctx* ctx, void* stream, const uint32_t* rayList, const uint32_t* counters,
                        const void* litScene, vqhip_format litFmt, int litPitchPx, const float* hierarchy,
                        const void* normals, vqhip_format normalFmt, int normalPitchPx,
                        const uint8_t* extractedRoughness, const uint8_t* blueNoise,
                        const VQ_SSSRConstants* cb, const vqhip_envmap* env,
                        void* radiance, vqhip_format radianceFmt, int radiancePitchPx) {
    vqk::Range range_("FFX SSSR Intersection");
    if (!ctx) return fail(nullptr, VQHIP_ERR_INVALID_ARG, "ssr_intersect: ctx is NULL");
    CTX_GUARD(ctx, "ssr_intersect");
    if (!rayList || !counters || !litScene || !hierarchy || !normals || !extractedRoughness || !blueNoise || !cb || !env || !radiance)
        return fail(ctx, VQHIP_ERR_INVALID_ARG, "ssr_intersect: NULL argument");
    int W, H;
    if (int rc = ssrFrame(ctx, "ssr_intersect", cb, " (the range of the depth hierarchy)", &W, &H)) return rc;
    if (!isImageFmt(litFmt) || !isImageFmt(radianceFmt)) return fail(ctx, VQHIP_ERR_UNSUPPORTED, "ssr_intersect: lit scene and radiance must be RGBA32F or RGBA16F");
    if (!isNormalFmt(normalFmt)) return fail(ctx, VQHIP_ERR_UNSUPPORTED, "ssr_intersect: normals must be R10G10B10A2_UNORM or RGBA32F");
    if (cb->maxTraversalIntersections > 256) return fail(ctx, VQHIP_ERR_UNSUPPORTED, "ssr_intersect: maxTraversalIntersections above 256 (the engine's slider range) is not supported");
    if (cb->mostDetailedMip > 5) return fail(ctx, VQHIP_ERR_UNSUPPORTED, "ssr_intersect: mostDetailedMip above 5 is not supported");
    if (badEnv(env)) return fail(ctx, VQHIP_ERR_INVALID_ARG, "ssr_intersect: env needs the specular cube and the BRDF LUT");
    const Plane planes[] = { { litScene, litPitchPx, imgBpp(litFmt), "" }, { radiance, radiancePitchPx, imgBpp(radianceFmt), "" }, { normals, normalPitchPx, nrmBpp(normalFmt), "" } };
    if (shortPitch(W, planes, 3)) return fail(ctx, VQHIP_ERR_INVALID_ARG, "ssr_intersect: pitch < width");
    const Span radianceSpan = spanOf(W, H, planes[1]);
    if (overlapsAny(spanOf(W, H, planes[0]), &radianceSpan, 1)) return fail(ctx, VQHIP_ERR_INVALID_ARG, "ssr_intersect: radiance overlaps the lit scene");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    SsrTraceArgs a;
    std::memset(&a, 0, sizeof(a));
    a.rayList = rayList; a.counters = counters; a.lit = litScene; a.mips = hierarchy; a.normals = normals; a.roughness = extractedRoughness; a.noise = blueNoise; a.out = radiance;
    a.width = W; a.height = H; a.litPitch = pitchOr(litPitchPx, W); a.normalPitch = pitchOr(normalPitchPx, W); a.outPitch = pitchOr(radiancePitchPx, W);
    a.litF32 = litFmt == VQHIP_FMT_RGBA32F; a.normF32 = normalFmt == VQHIP_FMT_RGBA32F; a.outF32 = radianceFmt == VQHIP_FMT_RGBA32F;
    a.levels = vqhip_mip_level_count(W, H);
    a.invViewProj = cb->invViewProjection; a.proj = cb->projection; a.invProj = cb->invProjection; a.view = cb->view; a.invView = cb->invView;
    copyEnvRotation(a.rot, cb);
    a.invDimX = cb->inverseBufferDimensions[0]; a.invDimY = cb->inverseBufferDimensions[1]; a.thickness = cb->depthBufferThickness;
    a.maxIter = cb->maxTraversalIntersections; a.minOcc = cb->minTraversalOccupancy; a.mostDetailedMip = cb->mostDetailedMip;
    a.pow5ExpLog = ctx->pow5ExpLog; a.arithDxc = ctx->arithDxc; a.env = *env;
    hipError_t e = launch_ssr_intersect((hipStream_t)stream, a, ctx->nCUs);
    return e == hipSuccess ? VQHIP_OK : failHip(ctx, e, "ssr_intersect launch");
}

// ---- SSR denoiser passes 2 and 3 (ssr_denoise.hip; docs/DESIGN_DETAILS.md §7.12) -----------------------------------------------------------
namespace {
// fills what both passes share and validates it; returns VQHIP_OK or the failure already recorded in ctx
int denoiseCommon(vqhip_ctx* ctx, const char* who, const VQ_SSSRConstants* cb, vqhip_format avgFmt, vqhip_format radianceFmt, vqhip_format outFmt,
                  const Plane* in, int nIn, const uint32_t* tileList, const uint32_t* counters, const void* avg, void* outRadiance, int outPitchPx, void* outVariance, int outVariancePitchPx, SsrDenoiseArgs* a) {
    const std::string w(who);
    int W, H;
    if (int rc = ssrFrame(ctx, who, cb, "", &W, &H)) return rc;
    if (!isImageFmt(radianceFmt) || !isImageFmt(outFmt)) return fail(ctx, VQHIP_ERR_UNSUPPORTED, w + ": radiance and output radiance must be RGBA32F or RGBA16F");
    if (!isAvgFmt(avgFmt)) return fail(ctx, VQHIP_ERR_UNSUPPORTED, w + ": the average radiance must be R11G11B10_FLOAT or RGBA32F");
    const Plane out[] = { { outRadiance, outPitchPx, imgBpp(outFmt), "" }, { outVariance, outVariancePitchPx, 2, "" } };
    if (shortPitch(W, out, 2) || shortPitch(W, in, nIn)) return fail(ctx, VQHIP_ERR_INVALID_ARG, w + ": pitch < width");
    const int tilesX = (W + 7) / 8, tilesY = (H + 7) / 8;
    const Span outs[] = { spanOf(W, H, out[0]), spanOf(W, H, out[1]) };
    if (overlapEachOther(outs, 2)) return fail(ctx, VQHIP_ERR_INVALID_ARG, w + ": the outputs overlap each other");
    if (const Plane* p = inputUnder(W, H, in, nIn, outs, 2))
        return fail(ctx, VQHIP_ERR_INVALID_ARG, w + ": an output overlaps the input " + p->name + " (the apron reads neighbours that other tiles write)");
    if (overlapsAny({ avg, (size_t)tilesX * tilesY * avgBpp(avgFmt), "" }, outs, 2)) return fail(ctx, VQHIP_ERR_INVALID_ARG, w + ": an output overlaps the input averageRadiance");
    if (tilesUnder(W, H, tileList, counters, outs, 2)) return fail(ctx, VQHIP_ERR_INVALID_ARG, w + ": an output overlaps the tile list or its counters");
    a->width = W; a->height = H; a->tilesX = tilesX; a->tilesY = tilesY; a->avgW = tilesX; a->avgH = tilesY;
    a->avg = avg; a->avgF32 = avgFmt == VQHIP_FMT_RGBA32F; a->radF32 = radianceFmt == VQHIP_FMT_RGBA32F; a->outF32 = outFmt == VQHIP_FMT_RGBA32F;
    a->outRadiance = outRadiance; a->outVariance = outVariance; a->outPitch = pitchOr(outPitchPx, W); a->outVariancePitch = pitchOr(outVariancePitchPx, W);
    a->arithDxc = ctx->arithDxc; a->roughnessThreshold = cb->roughnessThreshold; a->temporalStability = cb->temporalStabilityFactor;
    auto roundUp8 = [](uint32_t v) { return (v & ~7u) == v ? v : v + 8u; };                       // FFX_DNSR_Reflections_RoundUp8 as written
    a->roundUp8W = (float)roundUp8((uint32_t)W); a->roundUp8H = (float)roundUp8((uint32_t)H);
    return VQHIP_OK;
}
} // namespace

int vqhip_ssr_prefilter(vqhip_ctx* ctx, void* stream, const uint32_t* denoiserTileList, const uint32_t* counters,
                        const float* depth, int depthPitchPx, const void* normals, vqhip_format normalFmt, int normalPitchPx,
                        const uint8_t* extractedRoughness, const void* averageRadiance, vqhip_format avgFmt,
                        const void* radiance, vqhip_format radianceFmt, int radiancePitchPx, const void* variance, int variancePitchPx,
                        const VQ_SSSRConstants* cb, void* outRadiance, vqhip_format outFmt, int outPitchPx, void* outVariance, int outVariancePitchPx) {
    vqk::Range range_("FFX DNSR Prefilter");
    if (!ctx) return fail(nullptr, VQHIP_ERR_INVALID_ARG, "ssr_prefilter: ctx is NULL");
    CTX_GUARD(ctx, "ssr_prefilter");
    if (!denoiserTileList || !counters || !depth || !normals || !extractedRoughness || !averageRadiance || !radiance || !variance || !cb || !outRadiance || !outVariance)
        return fail(ctx, VQHIP_ERR_INVALID_ARG, "ssr_prefilter: NULL argument");
    if (!isNormalFmt(normalFmt)) return fail(ctx, VQHIP_ERR_UNSUPPORTED, "ssr_prefilter: normals must be R10G10B10A2_UNORM or RGBA32F");
    SsrDenoiseArgs a;
    std::memset(&a, 0, sizeof(a));
    const Plane in[] = { { depth, depthPitchPx, 4, "depth" }, { normals, normalPitchPx, nrmBpp(normalFmt), "normals" }, { extractedRoughness, 0, 1, "extractedRoughness" },
                         { radiance, radiancePitchPx, imgBpp(radianceFmt), "radiance" }, { variance, variancePitchPx, 2, "variance" } };
    int rc = denoiseCommon(ctx, "ssr_prefilter", cb, avgFmt, radianceFmt, outFmt, in, 5, denoiserTileList, counters, averageRadiance, outRadiance, outPitchPx, outVariance, outVariancePitchPx, &a);
    if (rc) return rc;
    const int W = a.width;
    a.tileList = denoiserTileList; a.counters = counters; a.depth = depth; a.normals = normals; a.roughness = extractedRoughness; a.radiance = radiance; a.variance = variance;
    a.depthPitch = pitchOr(depthPitchPx, W); a.normalPitch = pitchOr(normalPitchPx, W); a.radiancePitch = pitchOr(radiancePitchPx, W); a.variancePitch = pitchOr(variancePitchPx, W);
    a.normF32 = normalFmt == VQHIP_FMT_RGBA32F;
    for (int i = 0; i < 4; ++i) { a.ipZ[i] = cb->invProjection.m[i][2]; a.ipW[i] = cb->invProjection.m[i][3]; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipError_t e = launch_ssr_prefilter((hipStream_t)stream, a, ctx->nCUs);
    return e == hipSuccess ? VQHIP_OK : failHip(ctx, e, "ssr_prefilter launch");
}

int vqhip_ssr_resolve_temporal(vqhip_ctx* ctx, void* stream, const uint32_t* denoiserTileList, const uint32_t* counters,
                               const uint8_t* extractedRoughness, const void* averageRadiance, vqhip_format avgFmt,
                               const void* radiance, vqhip_format radianceFmt, int radiancePitchPx,
                               const void* reprojectedRadiance, vqhip_format reprojectedFmt, int reprojectedPitchPx,
                               const void* variance, int variancePitchPx, const void* sampleCount, int sampleCountPitchPx,
                               const VQ_SSSRConstants* cb, void* outRadiance, vqhip_format outFmt, int outPitchPx, void* outVariance, int outVariancePitchPx) {
    vqk::Range range_("FFX DNSR Resolve Temporal");
    if (!ctx) return fail(nullptr, VQHIP_ERR_INVALID_ARG, "ssr_resolve_temporal: ctx is NULL");
    CTX_GUARD(ctx, "ssr_resolve_temporal");
    if (!denoiserTileList || !counters || !extractedRoughness || !averageRadiance || !radiance || !reprojectedRadiance || !variance || !sampleCount || !cb || !outRadiance || !outVariance)
        return fail(ctx, VQHIP_ERR_INVALID_ARG, "ssr_resolve_temporal: NULL argument");
    if (!isImageFmt(reprojectedFmt)) return fail(ctx, VQHIP_ERR_UNSUPPORTED, "ssr_resolve_temporal: the reprojected radiance must be RGBA32F or RGBA16F");
    SsrDenoiseArgs a;
    std::memset(&a, 0, sizeof(a));
    const Plane in[] = { { extractedRoughness, 0, 1, "extractedRoughness" }, { radiance, radiancePitchPx, imgBpp(radianceFmt), "radiance" },
                         { reprojectedRadiance, reprojectedPitchPx, imgBpp(reprojectedFmt), "reprojectedRadiance" },
                         { variance, variancePitchPx, 2, "variance" }, { sampleCount, sampleCountPitchPx, 2, "sampleCount" } };
    int rc = denoiseCommon(ctx, "ssr_resolve_temporal", cb, avgFmt, radianceFmt, outFmt, in, 5, denoiserTileList, counters, averageRadiance, outRadiance, outPitchPx, outVariance, outVariancePitchPx, &a);
    if (rc) return rc;
    const int W = a.width;
    a.tileList = denoiserTileList; a.counters = counters; a.roughness = extractedRoughness; a.radiance = radiance; a.reprojected = reprojectedRadiance;
    a.variance = variance; a.sampleCount = sampleCount;
    a.radiancePitch = pitchOr(radiancePitchPx, W); a.reprojectedPitch = pitchOr(reprojectedPitchPx, W); a.variancePitch = pitchOr(variancePitchPx, W); a.sampleCountPitch = pitchOr(sampleCountPitchPx, W);
    a.reprojF32 = reprojectedFmt == VQHIP_FMT_RGBA32F;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipError_t e = launch_ssr_resolve_temporal((hipStream_t)stream, a, ctx->nCUs);
    return e == hipSuccess ? VQHIP_OK : failHip(ctx, e, "ssr_resolve_temporal launch");
}

// ---- SSR denoiser pass 1 (ssr_reproject.hip; docs/DESIGN_DETAILS.md §7.13) --------------------------------------------------------------------
int vqhip_ssr_reproject(vqhip_ctx* ctx, void* stream, const vqhip_ssr_reproject_surfaces* io, const VQ_SSSRConstants* cb) {
    vqk::Range range_("FFX DNSR Reproject");
    if (!ctx) return fail(nullptr, VQHIP_ERR_INVALID_ARG, "ssr_reproject: ctx is NULL");
    CTX_GUARD(ctx, "ssr_reproject");
    if (!io || !cb) return fail(ctx, VQHIP_ERR_INVALID_ARG, "ssr_reproject: NULL argument");
    if (!io->tile_list || !io->counters || !io->depth || !io->normals || !io->roughness || !io->depth_history || !io->normal_history || !io->roughness_history ||
        !io->radiance || !io->radiance_history || !io->motion_vectors || !io->variance_history || !io->sample_count_history ||
        !io->out_reprojected || !io->out_average || !io->out_variance || !io->out_sample_count)
        return fail(ctx, VQHIP_ERR_INVALID_ARG, "ssr_reproject: NULL plane");
    int W, H;
    if (int rc = ssrFrame(ctx, "ssr_reproject", cb, "", &W, &H)) return rc;
    if (!isNormalFmt(io->normals_fmt) || !isNormalFmt(io->normal_history_fmt)) return fail(ctx, VQHIP_ERR_UNSUPPORTED, "ssr_reproject: normals must be R10G10B10A2_UNORM or RGBA32F");
    if (!isImageFmt(io->radiance_fmt) || !isImageFmt(io->radiance_history_fmt) || !isImageFmt(io->out_reprojected_fmt))
        return fail(ctx, VQHIP_ERR_UNSUPPORTED, "ssr_reproject: radiance, its history and the reprojected radiance must be RGBA32F or RGBA16F");
    if (io->motion_fmt != VQHIP_FMT_RG16F && io->motion_fmt != VQHIP_FMT_RG32F) return fail(ctx, VQHIP_ERR_UNSUPPORTED, "ssr_reproject: motion vectors must be RG16F or RG32F");
    if (!isAvgFmt(io->out_average_fmt)) return fail(ctx, VQHIP_ERR_UNSUPPORTED, "ssr_reproject: the average radiance must be R11G11B10_FLOAT or RGBA32F");
    auto pitch = [&](int p) { return pitchOr(p, W); };
    const int tilesX = (W + 7) / 8, tilesY = (H + 7) / 8;
    const Plane in[] = { { io->depth, io->depth_pitch_px, 4, "depth" }, { io->normals, io->normals_pitch_px, nrmBpp(io->normals_fmt), "normals" },
                         { io->roughness, io->roughness_pitch_px, 1, "roughness" }, { io->depth_history, io->depth_history_pitch_px, 4, "depth_history" },
                         { io->normal_history, io->normal_history_pitch_px, nrmBpp(io->normal_history_fmt), "normal_history" },
                         { io->roughness_history, io->roughness_history_pitch_px, 1, "roughness_history" }, { io->radiance, io->radiance_pitch_px, imgBpp(io->radiance_fmt), "radiance" },
                         { io->radiance_history, io->radiance_history_pitch_px, imgBpp(io->radiance_history_fmt), "radiance_history" },
                         { io->motion_vectors, io->motion_pitch_px, motionBpp(io->motion_fmt), "motion_vectors" },
                         { io->variance_history, io->variance_history_pitch_px, 2, "variance_history" }, { io->sample_count_history, io->sample_count_history_pitch_px, 2, "sample_count_history" } };
    const Plane outFull[] = { { io->out_reprojected, io->out_reprojected_pitch_px, imgBpp(io->out_reprojected_fmt), "out_reprojected" },
                              { io->out_variance, io->out_variance_pitch_px, 2, "out_variance" }, { io->out_sample_count, io->out_sample_count_pitch_px, 2, "out_sample_count" } };
    for (const Plane* p : { shortPitch(W, in, 11), shortPitch(W, outFull, 3) })
        if (p) return fail(ctx, VQHIP_ERR_INVALID_ARG, std::string("ssr_reproject: pitch < width: ") + p->name);
    const Span outs[] = { spanOf(W, H, outFull[0]), spanOf(W, H, outFull[1]), spanOf(W, H, outFull[2]),
                          { io->out_average, (size_t)tilesX * tilesY * avgBpp(io->out_average_fmt), "out_average" } };
    if (overlapEachOther(outs, 4)) return fail(ctx, VQHIP_ERR_INVALID_ARG, "ssr_reproject: the outputs overlap each other");
    for (const Span& o : outs) {
        if (const Plane* p = inputUnder(W, H, in, 11, &o, 1))
            return fail(ctx, VQHIP_ERR_INVALID_ARG, std::string("ssr_reproject: ") + o.name + " overlaps the input " + p->name + " (tiles read what other tiles would write; ping-pong the history)");
        if (tilesUnder(W, H, io->tile_list, io->counters, &o, 1)) return fail(ctx, VQHIP_ERR_INVALID_ARG, std::string("ssr_reproject: ") + o.name + " overlaps the tile list or its counters");
    }
    SsrReprojectArgs a;
    std::memset(&a, 0, sizeof(a));
    a.tileList = io->tile_list; a.counters = io->counters; a.depth = io->depth; a.normals = io->normals; a.roughness = io->roughness;
    a.depthHist = io->depth_history; a.normalHist = io->normal_history; a.roughnessHist = io->roughness_history;
    a.radiance = io->radiance; a.radianceHist = io->radiance_history; a.motion = io->motion_vectors; a.varianceHist = io->variance_history; a.sampleCountHist = io->sample_count_history;
    a.outReprojected = io->out_reprojected; a.outAverage = io->out_average; a.outVariance = io->out_variance; a.outSampleCount = io->out_sample_count;
    a.width = W; a.height = H; a.tilesX = tilesX; a.tilesY = tilesY;
    a.depthPitch = pitch(io->depth_pitch_px); a.normalPitch = pitch(io->normals_pitch_px); a.roughnessPitch = pitch(io->roughness_pitch_px);
    a.depthHistPitch = pitch(io->depth_history_pitch_px); a.normalHistPitch = pitch(io->normal_history_pitch_px); a.roughnessHistPitch = pitch(io->roughness_history_pitch_px);
    a.radiancePitch = pitch(io->radiance_pitch_px); a.radianceHistPitch = pitch(io->radiance_history_pitch_px); a.motionPitch = pitch(io->motion_pitch_px);
    a.varianceHistPitch = pitch(io->variance_history_pitch_px); a.sampleCountHistPitch = pitch(io->sample_count_history_pitch_px);
    a.outReprojectedPitch = pitch(io->out_reprojected_pitch_px); a.outVariancePitch = pitch(io->out_variance_pitch_px); a.outSampleCountPitch = pitch(io->out_sample_count_pitch_px);
    a.normF32 = io->normals_fmt == VQHIP_FMT_RGBA32F; a.normHistF32 = io->normal_history_fmt == VQHIP_FMT_RGBA32F; a.radF32 = io->radiance_fmt == VQHIP_FMT_RGBA32F;
    a.radHistF32 = io->radiance_history_fmt == VQHIP_FMT_RGBA32F; a.motionF32 = io->motion_fmt == VQHIP_FMT_RG32F; a.outF32 = io->out_reprojected_fmt == VQHIP_FMT_RGBA32F;
    a.avgF32 = io->out_average_fmt == VQHIP_FMT_RGBA32F; a.arithDxc = ctx->arithDxc;
    a.invProj = cb->invProjection; a.invView = cb->invView; a.prevViewProj = cb->prevViewProjection; a.roughnessThreshold = cb->roughnessThreshold;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipError_t e = launch_ssr_reproject((hipStream_t)stream, a, ctx->nCUs);
    return e == hipSuccess ? VQHIP_OK : failHip(ctx, e, "ssr_reproject launch");
}

int vqhip_specular_mip_count(int spec_res0) { return vqhip_mip_level_count(spec_res0, spec_res0) - 1; }
size_t vqhip_cube_bytes(int res0, int nMips, vqhip_format fmt) {
    const size_t bpp = fmt == VQHIP_FMT_RGBA32F ? 16 : 8;
    size_t px = 0;
    for (int m = 0; m < nMips; ++m) { size_t r = (size_t)(res0 >> m); px += 6 * r * r; }
    return px * bpp;
}

static int checkChain(vqhip_ctx* ctx, const void* chain, int w0, int h0, int nMips, const char* who) {
    if (!ctx) return fail(nullptr, VQHIP_ERR_INVALID_ARG, std::string(who) + ": ctx is NULL");
    if (!chain || w0 <= 0 || h0 <= 0 || nMips <= 0 || nMips > vqhip_mip_level_count(w0, h0)) return fail(ctx, VQHIP_ERR_INVALID_ARG, std::string(who) + ": bad equirect chain");
    return VQHIP_OK;
}

int vqhip_conv_diffuse(vqhip_ctx* ctx, void* stream, const void* equirect_mips, int w0, int h0, int nMips,
                       int diffuseRes, float step, vqhip_conv_order order, void* outCube, vqhip_format fmt) {
    vqk::Range range_("DiffuseIrradianceCubemap");
    if (!ctx) return fail(nullptr, VQHIP_ERR_INVALID_ARG, "conv_diffuse: ctx is NULL");
    CTX_GUARD(ctx, "conv_diffuse");                          // before anything writes the context's error string
    int rc = checkChain(ctx, equirect_mips, w0, h0, nMips, "conv_diffuse");
    if (rc) return rc;
    if (!outCube || diffuseRes <= 0 || !(step > 0.0f)) return fail(ctx, VQHIP_ERR_INVALID_ARG, "conv_diffuse: bad argument");
    if (!isImageFmt(fmt)) return fail(ctx, VQHIP_ERR_UNSUPPORTED, "conv_diffuse: fmt must be RGBA32F or RGBA16F");
    if (order != VQHIP_CONV_SEQUENTIAL && order != VQHIP_CONV_WAVE64) return fail(ctx, VQHIP_ERR_INVALID_ARG, "conv_diffuse: bad order");
    // fp32 sequences of `for (phi = 0; phi < TWO_PI; phi += step)` / `for (theta = 0; theta < PI_OVER_TWO; theta += step)`
    // (CubemapConvolution.hlsl:132-136): plain IEEE adds, identical on any host.
    const size_t maxFloats = kConstSlotBytes / sizeof(float);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    int slot;
    rc = acquireSlot(ctx, &slot);
    if (rc) return rc;
    float* tab = (float*)(ctx->hostRing + (size_t)slot * kConstSlotBytes);
    size_t n = 0; int nPhi = 0, nTheta = 0;
    for (float phi = 0.0f; phi < 6.28318530718f; phi += step) { if (n >= maxFloats) return fail(ctx, VQHIP_ERR_UNSUPPORTED, "conv_diffuse: step too small"); tab[n++] = phi; ++nPhi; }
    for (float th = 0.0f; th < 1.5707963268f; th += step) { if (n >= maxFloats) return fail(ctx, VQHIP_ERR_UNSUPPORTED, "conv_diffuse: step too small"); tab[n++] = th; ++nTheta; }
    if ((size_t)nTheta * 2 * sizeof(float) > 60 * 1024) return fail(ctx, VQHIP_ERR_UNSUPPORTED, "conv_diffuse: step too small for the LDS theta table");
    rc = commitSlot(ctx, slot, n * sizeof(float), st);
    if (rc) return rc;
    const float* dtab = (const float*)(ctx->devRing + (size_t)slot * kConstSlotBytes);
    const size_t recNeed = conv_diffuse_record_bytes(w0, h0, nMips);
    if (recNeed) {
        if (ctx->recUsed) HIP_TRY(ctx, hipStreamWaitEvent(st, ctx->recFree, 0));
        if (ctx->recBytes < recNeed) {
            if (ctx->rec) { HIP_TRY(ctx, hipDeviceSynchronize()); HIP_TRY(ctx, hipFree(ctx->rec)); ctx->rec = nullptr; ctx->recBytes = 0; }
            HIP_TRY(ctx, hipMalloc(&ctx->rec, recNeed));
            ctx->recBytes = recNeed;
        }
        if (!ctx->recFree) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->recFree, hipEventDisableTiming));
    }
    hipError_t e = launch_conv_diffuse_tables(st, (const float4*)equirect_mips, w0, h0, nMips, diffuseRes, dtab, nPhi, dtab + nPhi, nTheta, order, outCube, fmt,
                                              recNeed ? ctx->rec : nullptr, ctx->opt);
    if (e != hipSuccess) return failHip(ctx, e, "conv_diffuse launch");
    if (recNeed) { HIP_TRY(ctx, hipEventRecord(ctx->recFree, st)); ctx->recUsed = true; }
    return releaseSlot(ctx, slot, st);
}

int vqhip_conv_specular(vqhip_ctx* ctx, void* stream, const void* equirect_mips, int w0, int h0, int nMips,
                        int specRes0, vqhip_conv_order order, void* outCubeMips, vqhip_format fmt) {
    vqk::Range range_("SpecularIrradianceCubemap");
    if (!ctx) return fail(nullptr, VQHIP_ERR_INVALID_ARG, "conv_specular: ctx is NULL");
    CTX_GUARD(ctx, "conv_specular");
    int rc = checkChain(ctx, equirect_mips, w0, h0, nMips, "conv_specular");
    if (rc) return rc;
    const int MIPS = vqhip_specular_mip_count(specRes0);
    if (!outCubeMips || specRes0 < 4 || (specRes0 & (specRes0 - 1)) || MIPS < 2) return fail(ctx, VQHIP_ERR_INVALID_ARG, "conv_specular: specRes0 must be a power of two >= 4");
    if (!isImageFmt(fmt)) return fail(ctx, VQHIP_ERR_UNSUPPORTED, "conv_specular: fmt must be RGBA32F or RGBA16F");
    if (order != VQHIP_CONV_SEQUENTIAL && order != VQHIP_CONV_WAVE64) return fail(ctx, VQHIP_ERR_INVALID_ARG, "conv_specular: bad order");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipError_t e = launch_conv_specular_all((hipStream_t)stream, (const float4*)equirect_mips, w0, h0, nMips, specRes0, MIPS, order, outCubeMips, fmt, ctx->opt);
    return e == hipSuccess ? VQHIP_OK : failHip(ctx, e, "conv_specular launch");
}

int vqhip_envmap_prefilter(vqhip_ctx* ctx, void* stream, const void* equirect_mips, int w0, int h0, int nMips,
                           int diffuseRes, float diffuseStep, int specRes0, vqhip_conv_order order, const vqhip_envmap_out* out) {
    vqk::Range range_("RenderEnvironmentMapCubeFaces");
    if (!ctx) return fail(nullptr, VQHIP_ERR_INVALID_ARG, "envmap_prefilter: ctx is NULL");
    CTX_GUARD(ctx, "envmap_prefilter");
    if (!out || !out->diffuse_blurred || !out->blur_tmp || !out->specular) return fail(ctx, VQHIP_ERR_INVALID_ARG, "envmap_prefilter: missing output buffer");
    void* diff = out->diffuse_unblurred;
    const size_t faceBytes = (size_t)diffuseRes * diffuseRes * 8;
    if (!diff) { int rc = ensureScratch(ctx, 6 * faceBytes); if (rc) return rc; diff = ctx->scratch; }
    int rc = vqhip_conv_diffuse(ctx, stream, equirect_mips, w0, h0, nMips, diffuseRes, diffuseStep, order, diff, VQHIP_FMT_RGBA16F);   // :181-277
    if (rc) return rc;
    VQ_BlurParams bp = { diffuseRes, diffuseRes };
    for (int face = 0; face < 6; ++face) {                                   // :279-373
        rc = vqhip_gaussian_blur_x(ctx, stream, (const char*)diff + face * faceBytes, out->blur_tmp, &bp, VQHIP_FMT_RGBA16F);
        if (rc) return rc;
        rc = vqhip_gaussian_blur_y(ctx, stream, out->blur_tmp, (char*)out->diffuse_blurred + face * faceBytes, nullptr, nullptr, 0, &bp, VQHIP_FMT_RGBA16F);
        if (rc) return rc;
    }
    return vqhip_conv_specular(ctx, stream, equirect_mips, w0, h0, nMips, specRes0, order, out->specular, VQHIP_FMT_RGBA16F);             // :386-472
}

// ---- FidelityFX CACAO at quality HIGH (cacao.hip; docs/DESIGN_DETAILS.md §7.14) ------------------------------------------------------------------
namespace {
struct CacaoLayout { size_t depth[4], normals, ping, pong, total; int hw, hh, mw[4], mh[4]; };
size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
bool cacaoLayout(int W, int H, CacaoLayout* L) {
    if (W <= 0 || H <= 0 || W > VQHIP_CACAO_MAX_DIM || H > VQHIP_CACAO_MAX_DIM) return false;
    L->hw = (W + 1) / 2; L->hh = (H + 1) / 2;
    size_t off = 0;
    for (int k = 0; k < 4; ++k) {
        L->mw[k] = mipDim(L->hw, k); L->mh[k] = mipDim(L->hh, k);
        L->depth[k] = off;
        off = align256(off + (size_t)4 * L->mw[k] * L->mh[k] * 2);
    }
    const size_t texels = (size_t)4 * L->hw * L->hh;
    L->normals = off; off = align256(off + texels * 4);
    L->ping = off;    off = align256(off + texels * 2);
    L->pong = off;    off = align256(off + texels * 2);
    L->total = off;
    return true;
}
} // namespace

size_t vqhip_cacao_work_bytes(int width, int height) {
    CacaoLayout L;
    return cacaoLayout(width, height, &L) ? L.total : 0;
}
size_t vqhip_cacao_plane_offset_bytes(int width, int height, int plane, int slice, int mip) {
    CacaoLayout L;
    if (!cacaoLayout(width, height, &L) || slice < 0 || slice > 3 || mip < 0 || mip > 3 || (plane != VQHIP_CACAO_PLANE_DEPTHS && mip != 0)) return 0;
    const size_t texels = (size_t)L.hw * L.hh;
    switch (plane) {
        case VQHIP_CACAO_PLANE_DEPTHS:  return L.depth[mip] + (size_t)slice * L.mw[mip] * L.mh[mip] * 2;
        case VQHIP_CACAO_PLANE_NORMALS: return L.normals + (size_t)slice * texels * 4;
        case VQHIP_CACAO_PLANE_PING:    return L.ping + (size_t)slice * texels * 2;
        case VQHIP_CACAO_PLANE_PONG:    return L.pong + (size_t)slice * texels * 2;
        default: return 0;
    }
}

// ---- FidelityFX CACAO at quality HIGHEST (cacao.hip; docs/DESIGN_DETAILS.md §7.15): HIGH's work layout as the prefix, three planes appended ------------------
namespace {
struct AdaptiveCacaoLayout { CacaoLayout high; size_t importance, importancePong, counter, total; int iw, ih; };
bool adaptiveCacaoLayout(int W, int H, AdaptiveCacaoLayout* L) {
    if (!cacaoLayout(W, H, &L->high)) return false;
    L->iw = (L->high.hw + 1) / 2; L->ih = (L->high.hh + 1) / 2;
    size_t off = L->high.total;
    L->importance = off;     off = align256(off + (size_t)L->iw * L->ih);
    L->importancePong = off; off = align256(off + (size_t)L->iw * L->ih);
    L->counter = off;        off = align256(off + 4);
    L->total = off;
    return true;
}
} // namespace

size_t vqhip_adaptive_cacao_work_bytes(int width, int height) {
    AdaptiveCacaoLayout L;
    return adaptiveCacaoLayout(width, height, &L) ? L.total : 0;
}
size_t vqhip_adaptive_cacao_plane_offset_bytes(int width, int height, int plane, int slice, int mip) {
    if (plane >= VQHIP_CACAO_PLANE_DEPTHS && plane <= VQHIP_CACAO_PLANE_PONG) return vqhip_cacao_plane_offset_bytes(width, height, plane, slice, mip);
    AdaptiveCacaoLayout L;
    if (!adaptiveCacaoLayout(width, height, &L) || slice != 0 || mip != 0) return 0;
    switch (plane) {
        case VQHIP_CACAO_PLANE_IMPORTANCE:      return L.importance;
        case VQHIP_CACAO_PLANE_IMPORTANCE_PONG: return L.importancePong;
        case VQHIP_CACAO_PLANE_LOAD_COUNTER:    return L.counter;
        default: return 0;
    }
}

// Both entry points behind their prologue: vqhip_cacao (adaptive false: `qualityLevel` must be HIGH, HIGH's work layout) and vqhip_adaptive_cacao (HIGHEST)
static int cacaoCall(vqhip_ctx* ctx, const char* who, bool adaptive, void* stream, const float* depth, size_t depthPitchBytes, const void* normals, int normalFmt,
        size_t normalPitchBytes, const VQ_CacaoConstants* shared, const VQ_CacaoConstants perPass[4], int qualityLevel, int blurPassCount,
        void* work, size_t workBytes, uint8_t* ao, size_t aoPitchBytes, int width, int height) {
    const std::string w(who);
    auto bad = [&](int code, const char* what) { return fail(ctx, code, w + ": " + what); };
    if (!depth || !normals || !shared || !perPass || !work || !ao) return bad(VQHIP_ERR_INVALID_ARG, "NULL argument");
    if (width <= 0 || height <= 0) return bad(VQHIP_ERR_INVALID_ARG, "bad dimensions");
    if (width > VQHIP_CACAO_MAX_DIM || height > VQHIP_CACAO_MAX_DIM) return bad(VQHIP_ERR_UNSUPPORTED, "frames above 16384 in either dimension are not supported");
    if (!adaptive) {
        if (qualityLevel < VQHIP_CACAO_QUALITY_LOWEST || qualityLevel > VQHIP_CACAO_QUALITY_HIGHEST) return bad(VQHIP_ERR_INVALID_ARG, "qualityLevel is not an FFX_CACAO_Quality");
        if (qualityLevel == VQHIP_CACAO_QUALITY_HIGHEST)
            return bad(VQHIP_ERR_UNSUPPORTED, "quality HIGHEST (the adaptive base pass, the importance map and the importance-driven tap loop) is vqhip_adaptive_cacao, with its larger work buffer; this entry point runs HIGH");
        if (qualityLevel != VQHIP_CACAO_QUALITY_HIGH) return bad(VQHIP_ERR_UNSUPPORTED, "quality levels LOWEST, LOW and MEDIUM are not implemented; use HIGH");
    }
    if (!isNormalFmt(normalFmt)) return bad(VQHIP_ERR_UNSUPPORTED, "normals must be R10G10B10A2_UNORM or RGBA32F");
    if (blurPassCount < 0 || blurPassCount > VQHIP_CACAO_MAX_BLUR_PASSES) return bad(VQHIP_ERR_INVALID_ARG, "blurPassCount must be 0..8");
    const size_t normalPx = normalFmt == VQHIP_FMT_RGBA32F ? 16 : 4;
    if (depthPitchBytes < (size_t)width * 4 || depthPitchBytes % 4) return bad(VQHIP_ERR_INVALID_ARG, "depthPitchBytes below 4 * width or not a multiple of 4");
    if (normalPitchBytes < (size_t)width * normalPx || normalPitchBytes % normalPx) return bad(VQHIP_ERR_INVALID_ARG, "normalPitchBytes below the row size or not a multiple of the pixel size");
    if (aoPitchBytes < (size_t)width) return bad(VQHIP_ERR_INVALID_ARG, "aoPitchBytes below the width");
    if (depthPitchBytes / 4 > 0x7fffffffu || normalPitchBytes / normalPx > 0x7fffffffu || aoPitchBytes > 0x7fffffffu) return bad(VQHIP_ERR_INVALID_ARG, "pitch too large");
    AdaptiveCacaoLayout A;                                                               // HIGH's layout is its prefix
    adaptiveCacaoLayout(width, height, &A);
    const CacaoLayout& L = A.high;
    const size_t total = adaptive ? A.total : L.total;
    if (workBytes < total) return fail(ctx, VQHIP_ERR_INVALID_ARG, w + ": workBytes below vqhip_" + w + "_work_bytes(width, height)");
    if ((uintptr_t)work % 256) return bad(VQHIP_ERR_INVALID_ARG, "work must be 256-byte aligned");
    // the constants must describe THIS frame, at HIGHEST the importance map included: the kernels address by the integer sizes and compute with the blocks' floats
    auto sizesMatch = [&](const VQ_CacaoConstants& c) {
        return c.SSAOBufferDimensions[0] == (float)L.hw && c.SSAOBufferDimensions[1] == (float)L.hh && c.DepthBufferDimensions[0] == (float)width &&
               c.DepthBufferDimensions[1] == (float)height && c.InputOutputBufferDimensions[0] == (float)width && c.InputOutputBufferDimensions[1] == (float)height &&
               c.DeinterleavedDepthBufferDimensions[0] == (float)L.hw && c.DeinterleavedDepthBufferDimensions[1] == (float)L.hh &&
               (!adaptive || (c.ImportanceMapDimensions[0] == (float)A.iw && c.ImportanceMapDimensions[1] == (float)A.ih));
    };
    if (!sizesMatch(*shared)) return bad(VQHIP_ERR_INVALID_ARG, "the shared constants are not those of this frame size at native resolution (FFX_CACAO_UpdateBufferSizeInfo(width, height, false))");
    for (int i = 0; i < 4; ++i) {
        if (!sizesMatch(perPass[i])) return bad(VQHIP_ERR_INVALID_ARG, "a per-pass constants block is not of this frame size at native resolution");
        if (perPass[i].PassIndex != i) return bad(VQHIP_ERR_INVALID_ARG, "perPass[i].PassIndex must be i");
    }
    const size_t depthBytes = (size_t)(height - 1) * depthPitchBytes + (size_t)width * 4, normalBytes = (size_t)(height - 1) * normalPitchBytes + (size_t)width * normalPx;
    const size_t aoBytes = (size_t)(height - 1) * aoPitchBytes + (size_t)width;
    if (rangesOverlap(work, total, depth, depthBytes) || rangesOverlap(work, total, normals, normalBytes) || rangesOverlap(work, total, ao, aoBytes) ||
        rangesOverlap(ao, aoBytes, depth, depthBytes) || rangesOverlap(ao, aoBytes, normals, normalBytes))
        return bad(VQHIP_ERR_INVALID_ARG, "work and ao must not overlap each other or the inputs");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    CacaoArgs a;
    std::memset(&a, 0, sizeof(a));
    a.depth = depth; a.normals = normals; a.work = (uint8_t*)work; a.ao = ao;
    for (int k = 0; k < 4; ++k) { a.offDepth[k] = L.depth[k]; a.mw[k] = L.mw[k]; a.mh[k] = L.mh[k]; }
    a.offNormals = L.normals; a.offPing = L.ping; a.offPong = L.pong;
    a.width = width; a.height = height; a.hw = L.hw; a.hh = L.hh;
    a.depthPitch = (int)(depthPitchBytes / 4); a.normalPitch = (int)(normalPitchBytes / normalPx); a.aoPitch = (int)aoPitchBytes;
    a.normF32 = normalFmt == VQHIP_FMT_RGBA32F; a.blurPasses = blurPassCount;
    const CacaoAdaptiveArgs ad = { A.importance, A.importancePong, A.counter, A.iw, A.ih };
    hipError_t e = adaptive ? launch_cacao_adaptive((hipStream_t)stream, a, ad, *shared, perPass) : launch_cacao((hipStream_t)stream, a, *shared, perPass);
    return e == hipSuccess ? VQHIP_OK : failHip(ctx, e, (w + " launch").c_str());
}

int vqhip_cacao(vqhip_ctx* ctx, void* stream, const float* depth, size_t depthPitchBytes, const void* normals, int normalFmt, size_t normalPitchBytes,
        const VQ_CacaoConstants* shared, const VQ_CacaoConstants perPass[4], int qualityLevel, int blurPassCount,
        void* work, size_t workBytes, uint8_t* ao, size_t aoPitchBytes, int width, int height) {
    vqk::Range range_("Ambient Occlusion (FidelityFX CACAO)");
    if (!ctx) return fail(nullptr, VQHIP_ERR_INVALID_ARG, "cacao: ctx is NULL");
    CTX_GUARD(ctx, "cacao");
    return cacaoCall(ctx, "cacao", false, stream, depth, depthPitchBytes, normals, normalFmt, normalPitchBytes, shared, perPass, qualityLevel, blurPassCount,
                     work, workBytes, ao, aoPitchBytes, width, height);
}

int vqhip_adaptive_cacao(vqhip_ctx* ctx, void* stream, const float* depth, size_t depthPitchBytes, const void* normals, int normalFmt, size_t normalPitchBytes,
        const VQ_CacaoConstants* shared, const VQ_CacaoConstants perPass[4], int blurPassCount,
        void* work, size_t workBytes, uint8_t* ao, size_t aoPitchBytes, int width, int height) {
    vqk::Range range_("Ambient Occlusion (FidelityFX CACAO)");
    if (!ctx) return fail(nullptr, VQHIP_ERR_INVALID_ARG, "adaptive_cacao: ctx is NULL");
    CTX_GUARD(ctx, "adaptive_cacao");
    return cacaoCall(ctx, "adaptive_cacao", true, stream, depth, depthPitchBytes, normals, normalFmt, normalPitchBytes, shared, perPass, VQHIP_CACAO_QUALITY_HIGHEST, blurPassCount,
                     work, workBytes, ao, aoPitchBytes, width, height);
}

// ---- The rasterisers' front ends (docs/DESIGN_DETAILS.md §7.16-7.20): what the eight entry points below share -------------------------------------------------
namespace {
extern "C++" {                                                 // templates and overloads: C++ linkage
constexpr size_t kRasterMaxDraws = 20000;                      // draws with indices in one call of any rasteriser
constexpr uint64_t kSceneMaxTriangles = (uint64_t)1 << 29;     // eight records each: the record counter is 32 bits wide; q stays far below 0xFFFFFFFF
template <class JOB> constexpr size_t slotsFor(size_t jobs) { return (jobs + kConstSlotBytes / sizeof(JOB) - 1) / (kConstSlotBytes / sizeof(JOB)); }   // ring slots a table takes

// What every rasteriser checks of a mesh draw, between its own NULL checks and its own cullMode / materialIndex / alignment / texture checks; empty = usable
std::string badMeshDraw(const vqhip_shadow_mesh& m, uint32_t numInstances, uint32_t minStride, uint32_t maxInstances) {
    if (m.indexBits != 16 && m.indexBits != 32) return "indexBits must be 16 or 32";
    if (m.numIndices % 3) return "numIndices is not a multiple of 3";
    if (m.strideBytes < minStride || m.strideBytes % 4) return "strideBytes below " + std::to_string(minStride) + " or not a multiple of 4";
    if (numInstances < 1 || numInstances > maxInstances) return "numInstances must be 1.." + std::to_string(maxInstances);
    return std::string();
}

// counters | boxes[fan n] | records[fan n] of a call that draws n instanced triangles; false above the rasteriser's limit or when the sizes do not fit
struct WorkLayout { uint64_t maxTriangles, fan; size_t counterBytes, boxBytes, recordBytes; };
constexpr WorkLayout kShadowLayout = { (uint64_t)1 << 40, 6, kRasterCounterBytes, kRasterBoxBytes, kRasterRecordBytes };
constexpr WorkLayout kSceneLayout = { kSceneMaxTriangles - 1, kSceneFanMax, kSceneCounterBytes, kSceneBoxBytes, kSceneRecordBytes };
bool workLayout(const WorkLayout& L, uint64_t instancedTriangles, size_t* boxes, size_t* records, size_t* total) {
    if (instancedTriangles > L.maxTriangles) return false;
    const uint64_t cap = instancedTriangles * L.fan;
    const uint64_t b = L.counterBytes, r = align256(b + cap * L.boxBytes), t = align256(r + cap * L.recordBytes);
    if (t > (uint64_t)SIZE_MAX) return false;
    *boxes = (size_t)b; *records = (size_t)r; *total = (size_t)t;
    return true;
}

// A host table of `count` JOBs through constant-ring slots, as many to a slot as it holds: per slot acquire, fill(job, k) for entry k = 0 .. n - 1 of the slot in
// host ring memory, commit sizeof(JOB) * n bytes, launch(the slot's device entries, n, entries staged before) — the ONE launch that reads the slot — and release.
// fill and launch own whatever runs across slots (the next draw, firstQ, firstMasked) or restarts in each (firstBlock: k == 0); launch returns a vqhip_status.
template <class JOB, class FILL, class LAUNCH>
int stageJobs(vqhip_ctx* ctx, hipStream_t st, size_t count, FILL&& fill, LAUNCH&& launch) {
    constexpr size_t perSlot = kConstSlotBytes / sizeof(JOB);
    static_assert(perSlot >= 1, "a ring slot holds at least one job");
    for (size_t done = 0; done < count;) {
        int slot;
        if (int rc = acquireSlot(ctx, &slot)) return rc;
        JOB* jobs = (JOB*)(ctx->hostRing + (size_t)slot * kConstSlotBytes);
        const size_t n = count - done < perSlot ? count - done : perSlot;
        for (size_t k = 0; k < n; ++k) fill(jobs[k], k);
        if (int rc = commitSlot(ctx, slot, sizeof(JOB) * n, st)) return rc;
        if (int rc = launch((const JOB*)(ctx->devRing + (size_t)slot * kConstSlotBytes), n, done)) return rc;
        if (int rc = releaseSlot(ctx, slot, st)) return rc;
        done += n;
    }
    return VQHIP_OK;
}
// the launch of a table that needs a home beyond its slots: k_table_copy of the slot's n entries to dst
template <class JOB>
int copySlotToTable(vqhip_ctx* ctx, hipStream_t st, const JOB* src, size_t n, JOB* dst, const std::string& who) {
    hipError_t e = launch_table_copy(st, src, dst, (uint32_t)(n * (sizeof(JOB) / 16)));
    return e == hipSuccess ? VQHIP_OK : failHip(ctx, e, (who + " table-copy launch").c_str());
}
// what a setup job takes of its draw's mesh; returns the draw's instanced triangles and takes its blocks of the slot's setup launch
template <class JOB, class DRAW>
uint64_t meshJob(JOB& J, const DRAW& D, uint64_t& blocks) {
    J.positions = (const uint8_t*)D.mesh.positions; J.indices = D.mesh.indices; J.wvp = D.matWorldViewProj;
    J.strideBytes = D.mesh.strideBytes; J.numVertices = D.mesh.numVertices; J.numTris = D.mesh.numIndices / 3; J.numInstances = D.numInstances;
    J.indexBits = D.mesh.indexBits; J.cullMode = D.cullMode; J.firstBlock = (uint32_t)blocks;
    const uint64_t tris = (uint64_t)J.numTris * J.numInstances;
    blocks += (tris + 255) / 256;
    return tris;
}

// ---- §7.19: what the masked entry points add to both rasterisers' host side ----
int hostTrunc(float x) { return x != x ? 0 : (int)(x < -2147483520.0f ? -2147483520.0f : x > 2147483520.0f ? 2147483520.0f : x); }     // vq_devmath.h f2i_trunc
const char* badMaskTexture(const vqhip_texture2d& t) {        // NULL = usable
    if (!t.texels) return nullptr;                             // a null SRV samples 0
    if (t.width < 1 || t.width > VQHIP_MASK_TEXTURE_MAX_DIM || t.height < 1 || t.height > VQHIP_MASK_TEXTURE_MAX_DIM) return "masked texture: width and height must be 1..16384";
    if (t.mips < 1 || t.mips > vqhip_mip_level_count(t.width, t.height)) return "masked texture: mips must be 1..vqhip_mip_level_count(width, height)";
    if ((uintptr_t)t.texels % 4) return "masked texture: texels must be 4-byte aligned";
    return nullptr;
}
// prefix | MaskTex[numDraws] | MaskSide[masked]; false when the sizes do not fit
bool maskLayout(size_t prefix, uint64_t instancedTriangles, uint64_t maskedTriangles, int numDraws, size_t* table, size_t* side, size_t* total) {
    if (!prefix || numDraws < 0 || maskedTriangles > instancedTriangles) return false;
    const uint64_t tb = prefix, sd = align256(tb + (uint64_t)(numDraws > 0 ? numDraws : 1) * sizeof(MaskTex)), t = align256(sd + maskedTriangles * sizeof(MaskSide));
    if (t > (uint64_t)SIZE_MAX) return false;
    *table = (size_t)tb; *side = (size_t)sd; *total = (size_t)t;
    return true;
}
// What the kernels' range guards rest on (vq_raster_mask.h loadMaskTri, the `at < sideCap` of both setup kernels: memory safety only — a guard that fired would
// draw a masked triangle solid, so these must hold): (1) a job's firstMasked is the running sum, ACROSS ring slots, of numTris * numInstances of the jobs before it
// whose maskSlot != 0, in the order the table was filled; (2) MaskArgs.sideCap is that sum over the whole call — sideTris in the scene call (draws that can discard),
// maskedTris in the shadow call (draws with a texture) — and never exceeds the masked count the work size was computed from; (3) 1 + the side index fits the
// record's 32-bit stamp: below 2^29 instanced triangles in a scene call, below 2^32 / 6 per view and 2^40 per call checked as 32 bits in a shadow call — the shadow
// call therefore refuses 2^32 - 1 or more masked instanced triangles; (4) MaskArgs.tableCap is the number of table entries staged, and maskSlot - 1 indexes them.
template <class JOB>
void maskJob(JOB& J, uint32_t maskSlot, uint64_t& firstMasked, uint64_t tris) {
    J.maskSlot = maskSlot; J.firstMasked = (uint32_t)firstMasked;
    if (maskSlot) firstMasked += tris;
}
// The MaskArgs of a call, all zero when no draw of it is alpha-tested; else its table goes into the work buffer, through ring slots (one k_table_copy launch per
// slot), as vqhip_scene_interpolants stages its draw table
int stageMask(vqhip_ctx* ctx, hipStream_t st, const std::vector<MaskTex>& table, void* work, size_t offTable, size_t offSide, uint64_t sideCap, const std::string& who, MaskArgs* ma) {
    std::memset(ma, 0, sizeof(*ma));
    if (table.empty()) return VQHIP_OK;
    MaskTex* dev = (MaskTex*)((char*)work + offTable);
    ma->table = dev; ma->side = (MaskSide*)((char*)work + offSide); ma->sideCap = sideCap; ma->tableCap = (uint32_t)table.size();
    size_t next = 0;
    return stageJobs<MaskTex>(ctx, st, table.size(), [&](MaskTex& t, size_t) { t = table[next++]; },
                              [&](const MaskTex* src, size_t n, size_t first) { return copySlotToTable(ctx, st, src, n, dev + first, who); });
}
// the two draw types of each rasteriser behind one set of accessors
const vqhip_shadow_draw& baseDraw(const vqhip_shadow_draw& d) { return d; }
const vqhip_shadow_draw& baseDraw(const vqhip_shadow_masked_draw& d) { return d.draw; }
const vqhip_texture2d* maskTexture(const vqhip_shadow_draw&) { return nullptr; }
const vqhip_texture2d* maskTexture(const vqhip_shadow_masked_draw& d) { return d.texDiffuseAlpha; }
const vqhip_scene_depth_draw& baseDraw(const vqhip_scene_depth_draw& d) { return d; }
const vqhip_scene_depth_draw& baseDraw(const vqhip_scene_masked_depth_draw& d) { return d.draw; }
const vqhip_material* maskMaterial(const vqhip_scene_depth_draw&) { return nullptr; }
const vqhip_material* maskMaterial(const vqhip_scene_masked_depth_draw& d) { return d.material && (d.material->texDiffuse.reserved & VQHIP_MATERIAL_ALPHA_MASKED) ? d.material : nullptr; }
} // extern "C++"
} // namespace

// ---- Shadow-map rasteriser (raster.hip; docs/DESIGN_DETAILS.md §7.16) --------------------------------------------------------------------------------------
// The view table's slot is held for the whole call: the mask table's and the jobs' slots must not lap the ring onto it
static_assert(sizeof(RasterView) * VQHIP_SHADOW_MAX_VIEWS <= kConstSlotBytes, "the view table fits one ring slot");
static_assert(slotsFor<RasterJob>(kRasterMaxDraws) + 1 < vqhip_ctx::kSlots, "one call never meets its own view-table slot again");
constexpr size_t kRasterMaxMaskedDraws = 10000;                // vqhip_shadow_masked_depth with a masked draw: table slots + job slots + the view table's stay inside the ring
static_assert(slotsFor<MaskTex>(kRasterMaxMaskedDraws) + slotsFor<RasterMaskedJob>(kRasterMaxMaskedDraws) + 1 < vqhip_ctx::kSlots, "one masked call never meets its own view-table slot again");

size_t vqhip_shadow_depth_work_bytes(uint64_t instancedTriangles, int numViews) {
    size_t b, r, t;
    if (numViews < 1 || numViews > VQHIP_SHADOW_MAX_VIEWS || !workLayout(kShadowLayout, instancedTriangles, &b, &r, &t)) return 0;
    return t;
}

// vqhip_shadow_depth (VIEW = vqhip_shadow_view) and vqhip_shadow_masked_depth (VIEW = vqhip_shadow_masked_view): one body, entered with the context guard held; `who` names the entry point in messages.
// A call without a masked draw enqueues exactly what vqhip_shadow_depth enqueues.
extern "C++" {
template <class VIEW>
int shadowDepthCall(vqhip_ctx* ctx, void* stream, const VIEW* views, int numViews, void* work, size_t workBytes, const std::string& who) {
    constexpr bool kMaskedEntry = !std::is_same<VIEW, vqhip_shadow_view>::value;
    vqk::Range range_("RenderShadowMaps");
    if (!views || !work) return fail(ctx, VQHIP_ERR_INVALID_ARG, who + ": NULL argument");
    if (numViews < 1 || numViews > VQHIP_SHADOW_MAX_VIEWS) return fail(ctx, VQHIP_ERR_INVALID_ARG, who + ": numViews must be 1..64");
    if ((uintptr_t)work % 256) return fail(ctx, VQHIP_ERR_INVALID_ARG, who + ": work must be 256-byte aligned");
    const int tile = ctx->opt.rasterTile ? ctx->opt.rasterTile : 32;
    auto bad = [&](int v, int d, const std::string& m) {
        return fail(ctx, VQHIP_ERR_INVALID_ARG, who + ": view " + std::to_string(v) + (d >= 0 ? " draw " + std::to_string(d) : std::string()) + ": " + m);
    };
    RasterView hv[VQHIP_SHADOW_MAX_VIEWS];
    uint64_t totalTris = 0, fillBlocks = 0, maskedTris = 0;
    size_t numJobs = 0, numDrawsAll = 0;
    std::vector<MaskTex> table;                                // one entry per masked draw with indices
    std::vector<uint32_t> slotOfJob;                           // per job (draw with indices), when the call has a masked draw: 1 + its table entry, or 0
    for (int v = 0; v < numViews; ++v) {
        const VIEW& V = views[v];
        if (!V.depth) return bad(v, -1, "depth is NULL");
        if (V.dim < 1 || V.dim > VQHIP_SHADOW_MAX_DIM) return bad(v, -1, "dim must be 1..8192");
        const size_t pitch = V.pitchBytes ? V.pitchBytes : (size_t)V.dim * 4;
        if (pitch < (size_t)V.dim * 4 || pitch % 4) return bad(v, -1, "pitchBytes below 4 * dim or not a multiple of 4");
        if (pitch / 4 > 0x7fffffffu) return bad(v, -1, "pitch too large");
        if ((uintptr_t)V.depth % 4) return bad(v, -1, "depth is not 4-byte aligned");
        if (V.numDraws < 0 || (V.numDraws > 0 && !V.draws)) return bad(v, -1, "numDraws < 0, or draws is NULL");
        if (V.linearDepth != 0 && V.linearDepth != 1) return bad(v, -1, "linearDepth must be 0 or 1");
        uint64_t viewTris = 0;
        for (int d = 0; d < V.numDraws; ++d) {
            const vqhip_shadow_draw& D = baseDraw(V.draws[d]);
            const vqhip_texture2d* tex = maskTexture(V.draws[d]);
            if (!D.mesh.positions || !D.mesh.indices || !D.matWorldViewProj) return bad(v, d, "positions, indices or matWorldViewProj is NULL");
            if (V.linearDepth && !D.matWorld) return bad(v, d, "matWorld is NULL in a linear-depth view");
            if (const std::string m = badMeshDraw(D.mesh, D.numInstances, 12, VQHIP_SHADOW_MAX_INSTANCES); !m.empty()) return bad(v, d, m);
            if (D.cullMode != VQHIP_CULL_NONE && D.cullMode != VQHIP_CULL_FRONT && D.cullMode != VQHIP_CULL_BACK) return bad(v, d, "unknown cullMode");
            if ((uintptr_t)D.mesh.positions % 4 || (uintptr_t)D.matWorldViewProj % 4 || (uintptr_t)D.matWorld % 4 || (uintptr_t)D.mesh.indices % (D.mesh.indexBits / 8))
                return bad(v, d, "positions / matrices must be 4-byte aligned, indices aligned to their size");
            if (tex) {
                if (D.mesh.strideBytes < 44) return bad(v, d, "a masked draw needs the engine's vertex (uv at byte 36): strideBytes below 44");
                if (const char* m = badMaskTexture(*tex)) return bad(v, d, m);
            }
            if (D.mesh.numIndices) {
                viewTris += (uint64_t)(D.mesh.numIndices / 3) * D.numInstances; ++numJobs;
                if (kMaskedEntry) {
                    slotOfJob.push_back(tex ? (uint32_t)table.size() + 1u : 0u);
                    if (tex) {
                        MaskTex t; std::memset(&t, 0, sizeof(t));
                        t.texels = tex->texels; t.width = tex->width; t.height = tex->height; t.mips = tex->mips; t.sx = t.sy = 1.0f;
                        table.push_back(t);
                        maskedTris += (uint64_t)(D.mesh.numIndices / 3) * D.numInstances;
                    }
                }
            }
        }
        numDrawsAll += (size_t)V.numDraws;
        RasterView& R = hv[v];
        std::memset(&R, 0, sizeof(R));
        R.depth = V.depth; R.pitch = (uint32_t)(pitch / 4); R.dim = V.dim; R.linear = V.linearDepth;
        R.recBase = totalTris * 6; R.recCap = viewTris * 6;
        R.cam[0] = V.cameraPosition.x; R.cam[1] = V.cameraPosition.y; R.cam[2] = V.cameraPosition.z; R.farPlane = V.farPlane;
        R.firstFillBlock = (uint32_t)fillBlocks;
        const uint64_t tiles = (uint64_t)((V.dim + tile - 1) / tile);
        fillBlocks += tiles * tiles;
        totalTris += viewTris;
        if (viewTris * 6 > 0xffffffffull) return fail(ctx, VQHIP_ERR_UNSUPPORTED, who + ": a view draws more than 2^32 / 6 instanced triangles");
    }
    if (numJobs > kRasterMaxDraws) return fail(ctx, VQHIP_ERR_UNSUPPORTED, who + ": more than 20000 draws in one call");
    if ((totalTris + 255) / 256 + numJobs > 0x7fffffffull) return fail(ctx, VQHIP_ERR_UNSUPPORTED, who + ": more than 2^31 triangle lanes in one call");
    size_t offBoxes, offRecords, need, offTable = 0, offSide = 0;
    bool fits = workLayout(kShadowLayout, totalTris, &offBoxes, &offRecords, &need);
    if (fits && kMaskedEntry) fits = numDrawsAll <= 0x7fffffffu && maskLayout(need, totalTris, maskedTris, (int)numDrawsAll, &offTable, &offSide, &need);
    if (!fits || workBytes < need)
        return fail(ctx, VQHIP_ERR_INVALID_ARG, who + (kMaskedEntry ? ": workBytes below vqhip_shadow_masked_depth_work_bytes(the call's instanced and masked instanced triangles, numViews, the views' draws)"
                                                                     : ": workBytes below vqhip_shadow_depth_work_bytes(the call's instanced triangles, numViews)"));
    const bool anyMasked = !table.empty();
    if (anyMasked && numJobs > kRasterMaxMaskedDraws) return fail(ctx, VQHIP_ERR_UNSUPPORTED, who + ": more than 10000 draws in one call that has a masked draw");
    if (maskedTris >= 0xffffffffull) return fail(ctx, VQHIP_ERR_UNSUPPORTED, who + ": 2^32 - 1 or more masked instanced triangles in one call");      // the record's 32-bit stamp
    for (int v = 0; v < numViews; ++v) {
        if (rangesOverlap(work, need, hv[v].depth, planeExtent((int)hv[v].dim, (int)hv[v].dim, hv[v].pitch, 4))) return bad(v, -1, "depth overlaps the work buffer");
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    uint32_t* counters = (uint32_t*)work;
    void* boxes = (char*)work + offBoxes;
    void* records = (char*)work + offRecords;
    int viewSlot;
    if (int rc = acquireSlot(ctx, &viewSlot)) return rc;
    std::memcpy(ctx->hostRing + (size_t)viewSlot * kConstSlotBytes, hv, sizeof(RasterView) * numViews);
    if (int rc = commitSlot(ctx, viewSlot, sizeof(RasterView) * numViews, st)) return rc;
    const RasterView* dviews = (const RasterView*)(ctx->devRing + (size_t)viewSlot * kConstSlotBytes);
    MaskArgs ma;
    if (int rc = stageMask(ctx, st, table, work, offTable, offSide, maskedTris, who, &ma)) return rc;
    hipError_t e = launch_raster_begin(st, counters, numViews);
    if (e != hipSuccess) return failHip(ctx, e, (who + " counters launch").c_str());
    // the draws that have indices, in ring slots of RasterJobs, or of the larger RasterMaskedJobs when a draw is masked: one setup launch per slot
    int v = 0, d = 0;
    size_t jobNo = 0;
    uint64_t blocks = 0, firstMasked = 0;
    auto fill = [&](auto& J, size_t k) {
        if (!k) blocks = 0;
        for (;;) {
            if (d >= views[v].numDraws) { ++v; d = 0; continue; }
            const vqhip_shadow_draw& D = baseDraw(views[v].draws[d++]);
            if (!D.mesh.numIndices) continue;
            J.world = D.matWorld; J.view = v;
            const uint64_t tris = meshJob(J, D, blocks);
            if constexpr (std::is_same<std::decay_t<decltype(J)>, RasterMaskedJob>::value) { maskJob(J, slotOfJob[jobNo], firstMasked, tris); J.pad[0] = J.pad[1] = 0u; }
            ++jobNo;
            return;
        }
    };
    auto setup = [&](const auto* jobs, size_t n, size_t, const auto&... mask) {
        hipError_t le = launch_raster_setup(st, jobs, (int)n, (uint32_t)blocks, dviews, counters, boxes, records, mask...);
        return le == hipSuccess ? VQHIP_OK : failHip(ctx, le, (who + " setup launch").c_str());
    };
    if (int rc = anyMasked ? stageJobs<RasterMaskedJob>(ctx, st, numJobs, fill, [&](const RasterMaskedJob* jobs, size_t n, size_t first) { return setup(jobs, n, first, ma); })
                           : stageJobs<RasterJob>(ctx, st, numJobs, fill, setup)) return rc;
    e = anyMasked ? launch_raster_fill(st, dviews, numViews, (uint32_t)fillBlocks, tile, counters, boxes, records, ma)
                  : launch_raster_fill(st, dviews, numViews, (uint32_t)fillBlocks, tile, counters, boxes, records);
    if (e != hipSuccess) return failHip(ctx, e, (who + " fill launch").c_str());
    return releaseSlot(ctx, viewSlot, st);
}
} // extern "C++"

int vqhip_shadow_depth(vqhip_ctx* ctx, void* stream, const vqhip_shadow_view* views, int numViews, void* work, size_t workBytes) {
    if (!ctx) return fail(nullptr, VQHIP_ERR_INVALID_ARG, "shadow_depth: ctx is NULL");
    CTX_GUARD(ctx, "shadow_depth");
    return shadowDepthCall(ctx, stream, views, numViews, work, workBytes, "shadow_depth");
}

size_t vqhip_shadow_masked_depth_work_bytes(uint64_t instancedTriangles, uint64_t maskedInstancedTriangles, int numViews, int numDraws) {
    size_t tb, sd, t;
    return maskLayout(vqhip_shadow_depth_work_bytes(instancedTriangles, numViews), instancedTriangles, maskedInstancedTriangles, numDraws, &tb, &sd, &t) ? t : 0;
}

int vqhip_shadow_masked_depth(vqhip_ctx* ctx, void* stream, const vqhip_shadow_masked_view* views, int numViews, void* work, size_t workBytes) {
    if (!ctx) return fail(nullptr, VQHIP_ERR_INVALID_ARG, "shadow_masked_depth: ctx is NULL");
    CTX_GUARD(ctx, "shadow_masked_depth");
    return shadowDepthCall(ctx, stream, views, numViews, work, workBytes, "shadow_masked_depth");
}

// ---- Main-view depth pre-pass (raster_view.hip; docs/DESIGN_DETAILS.md §7.17) ------------------------------------------------------------------------------------
static_assert(slotsFor<SceneDepthJob>(kRasterMaxDraws) < vqhip_ctx::kSlots, "one call never laps the ring");

size_t vqhip_scene_depth_work_bytes(uint64_t instancedTriangles) {
    size_t b, r, t;
    return workLayout(kSceneLayout, instancedTriangles, &b, &r, &t) ? t : 0;
}

// vqhip_scene_depth (DRAW = vqhip_scene_depth_draw) and vqhip_scene_masked_depth (DRAW = vqhip_scene_masked_depth_draw): one body, entered with the context guard held; `who` names the entry
// point in messages. A call without a masked draw enqueues exactly what vqhip_scene_depth enqueues.
extern "C++" {
template <class DRAW>
int sceneDepthCall(vqhip_ctx* ctx, void* stream, const DRAW* draws, int numDraws, int width, int height, int samples,
                   const vqhip_scene_depth_targets* out, void* work, size_t workBytes, const std::string& who) {
    constexpr bool kMaskedEntry = !std::is_same<DRAW, vqhip_scene_depth_draw>::value;
    vqk::Range range_("RenderDepthPrePass");
    auto bad = [&](const std::string& m) { return fail(ctx, VQHIP_ERR_INVALID_ARG, who + ": " + m); };
    if (!out || !out->depth || !work) return bad("NULL argument (out, out->depth or work)");
    if (numDraws < 0 || (numDraws > 0 && !draws)) return bad("numDraws < 0, or draws is NULL");
    if (samples != 1 && samples != 4) return bad("samples must be 1 or 4");
    if (width < 1 || width > VQHIP_SCENE_DEPTH_MAX_DIM || height < 1 || height > VQHIP_SCENE_DEPTH_MAX_DIM) return bad("width and height must be 1..8192");
    if (out->layers < 0 || out->layers > VQHIP_SCENE_DEPTH_MAX_LAYERS) return bad("layers must be 0..4");
    if (samples == 1 && out->layers != 0) return bad("layers are defined at samples == 4 only");
    if (out->reserved != 0) return bad("reserved must be 0");
    if (out->pitch < 0 || out->coverage_pitch < 0) return bad("negative pitch");
    const size_t pitch = out->pitch ? (size_t)out->pitch : (size_t)width, covPitch = out->coverage_pitch ? (size_t)out->coverage_pitch : (size_t)width;
    if (pitch < (size_t)width || covPitch < (size_t)width) return bad("a pitch below width");
    const size_t px = (size_t)samples * 4;                     // bytes per pixel of depth / primitive
    if ((uintptr_t)out->depth % px || (uintptr_t)out->primitive % px) return bad("depth / primitive must be 4-byte (samples 1) or 16-byte (samples 4) aligned");
    if ((uintptr_t)work % 256) return bad("work must be 256-byte aligned");
    for (int k = 0; k < out->layers; ++k) if ((uintptr_t)out->layerPrimitive[k] % 4) return bad("layerPrimitive must be 4-byte aligned");
    uint64_t totalTris = 0, maskedTris = 0, sideTris = 0;      // maskedTris: the header's rule (sizes the work buffer); sideTris: those that can discard
    size_t numJobs = 0;
    std::vector<MaskTex> table;                                // one entry per draw that can discard
    std::vector<uint32_t> slotOfJob;                           // per job (draw with indices), in a masked call: 1 + its table entry, or 0
    for (int d = 0; d < numDraws; ++d) {
        const vqhip_scene_depth_draw& D = baseDraw(draws[d]);
        const vqhip_material* mat = maskMaterial(draws[d]);
        auto badDraw = [&](const std::string& m) { return bad("draw " + std::to_string(d) + ": " + m); };
        if (!D.mesh.positions || !D.mesh.indices || !D.matWorldViewProj) return badDraw("positions, indices or matWorldViewProj is NULL");
        if (const std::string m = badMeshDraw(D.mesh, D.numInstances, 12, VQHIP_SCENE_DEPTH_MAX_INSTANCES); !m.empty()) return badDraw(m);
        if (D.cullMode != VQHIP_CULL_NONE && D.cullMode != VQHIP_CULL_FRONT && D.cullMode != VQHIP_CULL_BACK) return badDraw("unknown cullMode");
        if ((uintptr_t)D.mesh.positions % 4 || (uintptr_t)D.matWorldViewProj % 4 || (uintptr_t)D.mesh.indices % (D.mesh.indexBits / 8))
            return badDraw("positions / matrices must be 4-byte aligned, indices aligned to their size");
        if (mat) {
            if (D.mesh.strideBytes < 44) return badDraw("a masked draw needs the engine's vertex (uv at byte 36): strideBytes below 44");
            if (const char* m = badMaskTexture(mat->texDiffuse)) return badDraw(m);
        }
        if (D.mesh.numIndices) {
            const uint64_t tris = (uint64_t)(D.mesh.numIndices / 3) * D.numInstances;
            totalTris += tris; ++numJobs;
            if (kMaskedEntry) {
                // DepthPrePass.hlsl:159: discard iff HasDiffuseMap(textureConfig) && a < 0.01f — without the bit the masked PSO discards nothing: drawn as opaque
                const bool discards = mat && (hostTrunc(mat->data.textureConfig) & 1) > 0;
                slotOfJob.push_back(discards ? (uint32_t)table.size() + 1u : 0u);
                if (mat) maskedTris += tris;
                if (discards) {
                    MaskTex t; std::memset(&t, 0, sizeof(t));
                    t.texels = mat->texDiffuse.texels; t.width = mat->texDiffuse.width; t.height = mat->texDiffuse.height; t.mips = mat->texDiffuse.mips;
                    t.sx = mat->data.uvScaleOffset.x; t.sy = mat->data.uvScaleOffset.y; t.ox = mat->data.uvScaleOffset.z; t.oy = mat->data.uvScaleOffset.w;
                    table.push_back(t);
                    sideTris += tris;
                }
            }
        }
    }
    if (totalTris >= kSceneMaxTriangles) return fail(ctx, VQHIP_ERR_UNSUPPORTED, who + ": 2^29 or more instanced triangles in one call");
    if (numJobs > kRasterMaxDraws) return fail(ctx, VQHIP_ERR_UNSUPPORTED, who + ": more than 20000 draws in one call");
    size_t offBoxes, offRecords, need, offTable = 0, offSide = 0;
    bool fits = workLayout(kSceneLayout, totalTris, &offBoxes, &offRecords, &need);
    if (fits && kMaskedEntry) fits = maskLayout(need, totalTris, maskedTris, numDraws, &offTable, &offSide, &need);
    if (!fits || workBytes < need)
        return bad(kMaskedEntry ? "workBytes below vqhip_scene_masked_depth_work_bytes(the call's instanced and masked instanced triangles, numDraws)"
                                : "workBytes below vqhip_scene_depth_work_bytes(the call's instanced triangles)");
    const bool anyMasked = !table.empty();
    bool overlap = rangesOverlap(work, need, out->depth, planeExtent(width, height, pitch, px)) ||
                   (out->primitive && rangesOverlap(work, need, out->primitive, planeExtent(width, height, pitch, px)));
    for (int k = 0; k < out->layers; ++k)
        overlap = overlap || (out->coverage[k] && rangesOverlap(work, need, out->coverage[k], planeExtent(width, height, covPitch, 1))) ||
                  (out->layerPrimitive[k] && rangesOverlap(work, need, out->layerPrimitive[k], planeExtent(width, height, pitch, 4)));
    if (overlap) return bad("an output overlaps the work buffer");

    SceneDepthArgs a;
    std::memset(&a, 0, sizeof(a));
    a.depth = out->depth; a.primitive = out->primitive;
    for (int k = 0; k < out->layers; ++k) { a.coverage[k] = out->coverage[k]; a.layerPrimitive[k] = out->layerPrimitive[k]; }
    a.recCap = totalTris * kSceneFanMax; a.pitch = (uint32_t)pitch; a.coveragePitch = (uint32_t)covPitch;
    a.width = width; a.height = height; a.samples = samples; a.layers = out->layers;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    uint32_t* counter = (uint32_t*)work;
    void* boxes = (char*)work + offBoxes;
    void* records = (char*)work + offRecords;
    MaskArgs ma;
    if (int rc = stageMask(ctx, st, table, work, offTable, offSide, sideTris, who, &ma)) return rc;
    hipError_t e = launch_raster_begin(st, counter, 1);
    if (e != hipSuccess) return failHip(ctx, e, (who + " counter launch").c_str());
    // the draws that have indices, in ring slots of SceneDepthJobs: one setup launch per slot
    int d = 0;
    size_t jobNo = 0;
    uint64_t blocks = 0, firstQ = 0, firstMasked = 0;
    auto fill = [&](SceneDepthJob& J, size_t k) {
        if (!k) blocks = 0;
        while (!baseDraw(draws[d]).mesh.numIndices) ++d;
        J.firstQ = (uint32_t)firstQ;
        const uint64_t tris = meshJob(J, baseDraw(draws[d++]), blocks);
        firstQ += tris;
        maskJob(J, anyMasked ? slotOfJob[jobNo] : 0u, firstMasked, tris);
        ++jobNo;
    };
    auto setup = [&](const SceneDepthJob* jobs, size_t n, size_t) {
        hipError_t le = anyMasked ? launch_scene_setup(st, jobs, (int)n, (uint32_t)blocks, a, counter, boxes, records, ma)
                                  : launch_scene_setup(st, jobs, (int)n, (uint32_t)blocks, a, counter, boxes, records);
        return le == hipSuccess ? VQHIP_OK : failHip(ctx, le, (who + " setup launch").c_str());
    };
    if (int rc = stageJobs<SceneDepthJob>(ctx, st, numJobs, fill, setup)) return rc;
    e = anyMasked ? launch_scene_fill(st, a, scene_depth_tile(ctx->opt.rasterTile, samples), counter, boxes, records, ma)
                  : launch_scene_fill(st, a, scene_depth_tile(ctx->opt.rasterTile, samples), counter, boxes, records);
    return e == hipSuccess ? VQHIP_OK : failHip(ctx, e, (who + " fill launch").c_str());
}
} // extern "C++"

int vqhip_scene_depth(vqhip_ctx* ctx, void* stream, const vqhip_scene_depth_draw* draws, int numDraws, int width, int height, int samples,
                      const vqhip_scene_depth_targets* out, void* work, size_t workBytes) {
    if (!ctx) return fail(nullptr, VQHIP_ERR_INVALID_ARG, "scene_depth: ctx is NULL");
    CTX_GUARD(ctx, "scene_depth");
    return sceneDepthCall(ctx, stream, draws, numDraws, width, height, samples, out, work, workBytes, "scene_depth");
}

size_t vqhip_scene_masked_depth_work_bytes(uint64_t instancedTriangles, uint64_t maskedInstancedTriangles, int numDraws) {
    size_t tb, sd, t;
    return maskLayout(vqhip_scene_depth_work_bytes(instancedTriangles), instancedTriangles, maskedInstancedTriangles, numDraws, &tb, &sd, &t) ? t : 0;
}

int vqhip_scene_masked_depth(vqhip_ctx* ctx, void* stream, const vqhip_scene_masked_depth_draw* draws, int numDraws, int width, int height, int samples,
                             const vqhip_scene_depth_targets* out, void* work, size_t workBytes) {
    if (!ctx) return fail(nullptr, VQHIP_ERR_INVALID_ARG, "scene_masked_depth: ctx is NULL");
    CTX_GUARD(ctx, "scene_masked_depth");
    return sceneDepthCall(ctx, stream, draws, numDraws, width, height, samples, out, work, workBytes, "scene_masked_depth");
}

// ---- The lit draw's interpolants from meshes (raster_attr.hip; docs/DESIGN_DETAILS.md §7.18) ----------------------------------------------------------------------
// A call of 20 000 draws may take more slots than the ring has (slotsFor<SurfaceJob>(kRasterMaxDraws) of them): acquireSlot then waits for the table copy that last
// read the slot, which this call enqueued.
size_t vqhip_scene_interpolants_work_bytes(int numDraws) {
    if (numDraws < 0) return 0;
    return align256((size_t)(numDraws > 0 ? numDraws : 1) * sizeof(SurfaceJob));
}

// vqhip_scene_interpolants (quadOut == NULL) and vqhip_scene_quad_interpolants (§7.20 Q1): one body, the launch differs
static int sceneInterpolants(vqhip_ctx* ctx, const std::string& w, void* stream, const vqhip_scene_surface_draw* draws, int numDraws, int width, int height,
                             const uint32_t* owner, int owner_pitch_px, const vqhip_scene_interpolant_targets* out, const vqhip_scene_quad_targets* quadOut,
                             void* work, size_t workBytes) {
    vqk::Range range_("RenderSceneColor");
    auto bad = [&](const std::string& m) { return fail(ctx, VQHIP_ERR_INVALID_ARG, w + ": " + m); };
    if (!out || !out->ip0 || !out->ip1 || !out->ip2 || !owner || !work) return bad("NULL argument (out, ip0, ip1, ip2, owner or work)");
    if (quadOut && !quadOut->quadUV) return bad("quadUV is NULL");
    if (numDraws < 0 || (numDraws > 0 && !draws)) return bad("numDraws < 0, or draws is NULL");
    if (!out->svPositionCurr != !out->svPositionPrev) return bad("svPositionCurr and svPositionPrev: both or neither");
    const bool sv = out->svPositionCurr != nullptr;
    if (width < 1 || width > VQHIP_SCENE_DEPTH_MAX_DIM || height < 1 || height > VQHIP_SCENE_DEPTH_MAX_DIM) return bad("width and height must be 1..8192");
    if (out->pitch < 0 || out->sv_pitch < 0 || owner_pitch_px < 0) return bad("negative pitch");
    const size_t pitch = out->pitch ? (size_t)out->pitch : (size_t)width, svPitch = out->sv_pitch ? (size_t)out->sv_pitch : (size_t)width;
    const size_t ownerPitch = owner_pitch_px ? (size_t)owner_pitch_px : (size_t)width;
    if (quadOut && quadOut->quad_pitch < 0) return bad("negative pitch");
    const size_t quadPitch = quadOut && quadOut->quad_pitch ? (size_t)quadOut->quad_pitch : (size_t)width;
    if (pitch < (size_t)width || svPitch < (size_t)width || ownerPitch < (size_t)width || quadPitch < (size_t)width) return bad("a pitch below width");
    void* const planes[6] = { out->ip0, out->ip1, out->ip2, out->svPositionCurr, out->svPositionPrev, quadOut ? quadOut->quadUV : nullptr };
    for (int k = 0; k < 6; ++k) if ((uintptr_t)planes[k] % 16) return bad("a target is not 16-byte aligned");
    if ((uintptr_t)owner % 4) return bad("owner must be 4-byte aligned");
    if ((uintptr_t)work % 256) return bad("work must be 256-byte aligned");
    uint64_t totalTris = 0;
    size_t numJobs = 0;
    for (int d = 0; d < numDraws; ++d) {
        const vqhip_scene_surface_draw& D = draws[d];
        auto badDraw = [&](const std::string& m) { return bad("draw " + std::to_string(d) + ": " + m); };
        if (!D.mesh.positions || !D.mesh.indices || !D.matWorldViewProj || !D.matWorld || !D.matNormal)
            return badDraw("positions, indices, matWorldViewProj, matWorld or matNormal is NULL");
        if (sv && !D.matWorldViewProjPrev) return badDraw("matWorldViewProjPrev is NULL while the sv planes are asked for");
        if (const std::string m = badMeshDraw(D.mesh, D.numInstances, 44, VQHIP_SCENE_DEPTH_MAX_INSTANCES); !m.empty()) return badDraw(m);
        if (D.materialIndex < 0) return badDraw("materialIndex is negative");
        if ((uintptr_t)D.mesh.positions % 4 || (uintptr_t)D.matWorldViewProj % 4 || (uintptr_t)D.matWorld % 4 || (uintptr_t)D.matNormal % 4 ||
            (uintptr_t)D.matWorldViewProjPrev % 4 || (uintptr_t)D.mesh.indices % (D.mesh.indexBits / 8))
            return badDraw("positions / matrices must be 4-byte aligned, indices aligned to their size");
        if (D.mesh.numIndices) { totalTris += (uint64_t)(D.mesh.numIndices / 3) * D.numInstances; ++numJobs; }
    }
    if (totalTris >= kSceneMaxTriangles) return fail(ctx, VQHIP_ERR_UNSUPPORTED, w + ": 2^29 or more instanced triangles in one call");
    if (numJobs > kRasterMaxDraws) return fail(ctx, VQHIP_ERR_UNSUPPORTED, w + ": more than 20000 draws in one call");
    const size_t need = vqhip_scene_interpolants_work_bytes(numDraws);
    if (workBytes < need) return bad("workBytes below vqhip_scene_interpolants_work_bytes(numDraws)");
    const size_t ownerBytes = planeExtent(width, height, ownerPitch, 4);
    const size_t quadBytes = planeExtent(width, height, quadPitch, 16);
    for (int k = 0; k < 6; ++k) {
        if (!planes[k]) continue;
        const size_t bytes = k == 5 ? quadBytes : planeExtent(width, height, k < 3 ? pitch : svPitch, 16);
        if (rangesOverlap(work, need, planes[k], bytes)) return bad("an output overlaps the work buffer");
        if (rangesOverlap(owner, ownerBytes, planes[k], bytes)) return bad("an output overlaps the owner plane");
        if (k < 5 && rangesOverlap(planes[5], quadBytes, planes[k], bytes)) return bad("quadUV overlaps another output");
    }

    SceneInterpArgs a;
    std::memset(&a, 0, sizeof(a));
    a.owner = owner; a.ip[0] = out->ip0; a.ip[1] = out->ip1; a.ip[2] = out->ip2; a.sv[0] = out->svPositionCurr; a.sv[1] = out->svPositionPrev;
    a.ownerPitch = (uint32_t)ownerPitch; a.pitch = (uint32_t)pitch; a.svPitch = (uint32_t)svPitch;
    a.width = width; a.height = height; a.numJobs = (int32_t)numJobs; a.totalTris = (uint32_t)totalTris;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    SurfaceJob* table = (SurfaceJob*)work;
    // the draws that have indices, in ring slots of SurfaceJobs: one table-copy launch per slot
    int d = 0;
    uint64_t firstQ = 0;
    auto fill = [&](SurfaceJob& J, size_t) {
        while (!draws[d].mesh.numIndices) ++d;
        const vqhip_scene_surface_draw& D = draws[d++];
        std::memset(&J, 0, sizeof(J));
        J.vertices = (const uint8_t*)D.mesh.positions; J.indices = D.mesh.indices;
        J.wvp = D.matWorldViewProj; J.world = D.matWorld; J.normal = D.matNormal; J.wvpPrev = D.matWorldViewProjPrev;
        J.strideBytes = D.mesh.strideBytes; J.numVertices = D.mesh.numVertices; J.numTris = D.mesh.numIndices / 3; J.numInstances = D.numInstances;
        J.indexBits = D.mesh.indexBits; J.materialIndex = D.materialIndex; J.firstQ = (uint32_t)firstQ;
        firstQ += (uint64_t)J.numTris * J.numInstances;
    };
    if (int rc = stageJobs<SurfaceJob>(ctx, st, numJobs, fill, [&](const SurfaceJob* src, size_t n, size_t first) { return copySlotToTable(ctx, st, src, n, table + first, w); })) return rc;
    const bool waveForm = ctx->opt.interpForm != 1;                                           // default: the wave form
    const QuadPlane qp = { planes[5], (uint32_t)quadPitch };
    hipError_t e = quadOut ? launch_scene_quad_interpolants(st, a, table, waveForm, qp) : launch_scene_interpolants(st, a, table, waveForm);
    return e == hipSuccess ? VQHIP_OK : failHip(ctx, e, (w + " launch").c_str());
}
int vqhip_scene_interpolants(vqhip_ctx* ctx, void* stream, const vqhip_scene_surface_draw* draws, int numDraws, int width, int height,
                             const uint32_t* owner, int owner_pitch_px, const vqhip_scene_interpolant_targets* out, void* work, size_t workBytes) {
    if (!ctx) return fail(nullptr, VQHIP_ERR_INVALID_ARG, "scene_interpolants: ctx is NULL");
    CTX_GUARD(ctx, "scene_interpolants");
    return sceneInterpolants(ctx, "scene_interpolants", stream, draws, numDraws, width, height, owner, owner_pitch_px, out, nullptr, work, workBytes);
}
int vqhip_scene_quad_interpolants(vqhip_ctx* ctx, void* stream, const vqhip_scene_surface_draw* draws, int numDraws, int width, int height,
                                  const uint32_t* owner, int owner_pitch_px, const vqhip_scene_quad_targets* out, void* work, size_t workBytes) {
    if (!ctx) return fail(nullptr, VQHIP_ERR_INVALID_ARG, "scene_quad_interpolants: ctx is NULL");
    CTX_GUARD(ctx, "scene_quad_interpolants");
    if (!out) return fail(ctx, VQHIP_ERR_INVALID_ARG, "scene_quad_interpolants: NULL argument (out, ip0, ip1, ip2, owner or work)");
    return sceneInterpolants(ctx, "scene_quad_interpolants", stream, draws, numDraws, width, height, owner, owner_pitch_px, &out->planes, out, work, workBytes);
}

// ---- The ObjectID pass's target from an owner plane (raster_ids.hip; docs/DESIGN_DETAILS.md §7.21 P0) ---------------------------------------------------------------
size_t vqhip_object_ids_work_bytes(int numDraws) {
    if (numDraws < 0) return 0;
    return align256((size_t)(numDraws > 0 ? numDraws : 1) * sizeof(ObjectIdJob));
}

int vqhip_object_ids(vqhip_ctx* ctx, void* stream, const vqhip_object_id_draw* draws, int numDraws, int width, int height,
                     const uint32_t* owner, int owner_pitch_px, int32_t* ids, int ids_pitch_px, void* work, size_t workBytes) {
    if (!ctx) return fail(nullptr, VQHIP_ERR_INVALID_ARG, "object_ids: ctx is NULL");
    CTX_GUARD(ctx, "object_ids");
    vqk::Range range_("RenderObjectIDPass");
    const std::string w = "object_ids";
    auto bad = [&](const std::string& m) { return fail(ctx, VQHIP_ERR_INVALID_ARG, w + ": " + m); };
    if (!owner || !ids || !work) return bad("NULL argument (owner, ids or work)");
    if (numDraws < 0 || (numDraws > 0 && !draws)) return bad("numDraws < 0, or draws is NULL");
    if (width < 1 || width > VQHIP_SCENE_DEPTH_MAX_DIM || height < 1 || height > VQHIP_SCENE_DEPTH_MAX_DIM) return bad("width and height must be 1..8192");
    if (owner_pitch_px < 0 || ids_pitch_px < 0) return bad("negative pitch");
    const size_t ownerPitch = owner_pitch_px ? (size_t)owner_pitch_px : (size_t)width, idsPitch = ids_pitch_px ? (size_t)ids_pitch_px : (size_t)width;
    if (ownerPitch < (size_t)width || idsPitch < (size_t)width) return bad("a pitch below width");
    if ((uintptr_t)ids % 16) return bad("ids is not 16-byte aligned");
    if ((uintptr_t)owner % 4) return bad("owner must be 4-byte aligned");
    if ((uintptr_t)work % 256) return bad("work must be 256-byte aligned");
    uint64_t totalTris = 0;
    size_t numJobs = 0;
    for (int d = 0; d < numDraws; ++d) {
        const vqhip_object_id_draw& D = draws[d];
        auto badDraw = [&](const std::string& m) { return bad("draw " + std::to_string(d) + ": " + m); };
        if (!D.objID) return badDraw("objID is NULL");
        if ((uintptr_t)D.objID % 4) return badDraw("objID must be 4-byte aligned");
        if (D.numIndices % 3) return badDraw("numIndices is not a multiple of 3");
        if (D.numInstances < 1 || D.numInstances > VQHIP_SCENE_DEPTH_MAX_INSTANCES) return badDraw("numInstances must be 1..64");
        if (D.numIndices) { totalTris += (uint64_t)(D.numIndices / 3) * D.numInstances; ++numJobs; }
    }
    if (totalTris >= kSceneMaxTriangles) return fail(ctx, VQHIP_ERR_UNSUPPORTED, w + ": 2^29 or more instanced triangles in one call");
    if (numJobs > kRasterMaxDraws) return fail(ctx, VQHIP_ERR_UNSUPPORTED, w + ": more than 20000 draws in one call");
    const size_t need = vqhip_object_ids_work_bytes(numDraws);
    if (workBytes < need) return bad("workBytes below vqhip_object_ids_work_bytes(numDraws)");
    const size_t ownerBytes = planeExtent(width, height, ownerPitch, 4), idsBytes = planeExtent(width, height, idsPitch, 16);
    if (rangesOverlap(work, need, ids, idsBytes)) return bad("ids overlaps the work buffer");
    if (rangesOverlap(owner, ownerBytes, ids, idsBytes)) return bad("ids overlaps the owner plane");

    ObjectIdArgs a;
    std::memset(&a, 0, sizeof(a));
    a.owner = owner; a.ids = ids; a.ownerPitch = (uint32_t)ownerPitch; a.idsPitch = (uint32_t)idsPitch;
    a.width = width; a.height = height; a.numJobs = (int32_t)numJobs; a.totalTris = (uint32_t)totalTris;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    ObjectIdJob* table = (ObjectIdJob*)work;
    // the draws that have indices, in ring slots of ObjectIdJobs: one table-copy launch per slot
    int d = 0;
    uint64_t firstQ = 0;
    auto fill = [&](ObjectIdJob& J, size_t) {
        while (!draws[d].numIndices) ++d;
        const vqhip_object_id_draw& D = draws[d++];
        std::memset(&J, 0, sizeof(J));
        J.objID = D.objID; J.numTris = D.numIndices / 3; J.numInstances = D.numInstances; J.meshID = D.meshID; J.materialID = D.materialID;
        J.firstQ = (uint32_t)firstQ;
        firstQ += (uint64_t)J.numTris * J.numInstances;
    };
    if (int rc = stageJobs<ObjectIdJob>(ctx, st, numJobs, fill, [&](const ObjectIdJob* src, size_t n, size_t first) { return copySlotToTable(ctx, st, src, n, table + first, w); })) return rc;
    // default: the wave form from 2^22 pixels on, the lane form below (profiles/r22a_editor_passes.md: 41.7 against 45.1 us at 3840 x 2160, 28.1 against 21.0 us at 1920 x 1080)
    const bool waveForm = ctx->opt.interpForm ? ctx->opt.interpForm != 1 : (uint64_t)width * (uint64_t)height >= ((uint64_t)1 << 22);
    hipError_t e = launch_object_ids(st, a, table, waveForm);
    return e == hipSuccess ? VQHIP_OK : failHip(ctx, e, (w + " launch").c_str());
}

// ---- The Outline pass (raster_outline.hip; docs/DESIGN_DETAILS.md §7.21 O1 .. O6) ----------------------------------------------------------------------------------
static_assert(slotsFor<OutlineJob>(kRasterMaxDraws) < vqhip_ctx::kSlots, "one call never laps the ring");
static constexpr uint64_t kOutlineMaxTriangles = (uint64_t)1 << 28;   // sixteen records each: the record counter is 32 bits wide
// counter | OutlineColor[min(triangles, max draws), at least 1] | boxes[16 n] | records[16 n]; false above the limit or when the sizes do not fit
static bool outlineLayout(uint64_t triangles, size_t* colors, size_t* colorCap, size_t* boxes, size_t* records, size_t* total) {
    if (triangles >= kOutlineMaxTriangles) return false;
    const uint64_t cap = triangles * kOutlineFanMax, nc = triangles < kRasterMaxDraws ? (triangles ? triangles : 1) : kRasterMaxDraws;
    const uint64_t c = kOutlineCounterBytes, b = align256(c + nc * sizeof(OutlineColor)), r = align256(b + cap * kOutlineBoxBytes), t = align256(r + cap * kOutlineRecordBytes);
    if (t > (uint64_t)SIZE_MAX) return false;
    *colors = (size_t)c; *colorCap = (size_t)nc; *boxes = (size_t)b; *records = (size_t)r; *total = (size_t)t;
    return true;
}

size_t vqhip_outline_work_bytes(uint64_t triangles) {
    size_t c, nc, b, r, t;
    return outlineLayout(triangles, &c, &nc, &b, &r, &t) ? t : 0;
}

int vqhip_outline(vqhip_ctx* ctx, void* stream, const vqhip_outline_draw* draws, int numDraws, int width, int height,
                  const vqhip_outline_targets* out, void* work, size_t workBytes) {
    if (!ctx) return fail(nullptr, VQHIP_ERR_INVALID_ARG, "outline: ctx is NULL");
    CTX_GUARD(ctx, "outline");
    vqk::Range range_("RenderOutline");
    const std::string w = "outline";
    auto bad = [&](const std::string& m) { return fail(ctx, VQHIP_ERR_INVALID_ARG, w + ": " + m); };
    if (!out || !out->sceneColor || !work) return bad("NULL argument (out, out->sceneColor or work)");
    if (numDraws < 0 || (numDraws > 0 && !draws)) return bad("numDraws < 0, or draws is NULL");
    if (width < 1 || width > VQHIP_SCENE_DEPTH_MAX_DIM || height < 1 || height > VQHIP_SCENE_DEPTH_MAX_DIM) return bad("width and height must be 1..8192");
    if (out->reserved != 0) return bad("reserved must be 0");
    if (out->pitch < 0 || out->selection_pitch < 0 || out->writer_pitch < 0) return bad("negative pitch");
    const size_t pitch = out->pitch ? (size_t)out->pitch : (size_t)width, selPitch = out->selection_pitch ? (size_t)out->selection_pitch : (size_t)width;
    const size_t wrPitch = out->writer_pitch ? (size_t)out->writer_pitch : (size_t)width;
    if (pitch < (size_t)width || selPitch < (size_t)width || wrPitch < (size_t)width) return bad("a pitch below width");
    if ((uintptr_t)out->sceneColor % 8) return bad("sceneColor is not 8-byte aligned");
    if ((uintptr_t)out->writer % 4) return bad("writer must be 4-byte aligned");
    if ((uintptr_t)work % 256) return bad("work must be 256-byte aligned");
    uint64_t totalTris = 0;
    size_t numJobs = 0;
    for (int d = 0; d < numDraws; ++d) {
        const vqhip_outline_draw& D = draws[d];
        auto badDraw = [&](const std::string& m) { return bad("draw " + std::to_string(d) + ": " + m); };
        if (!D.mesh.positions || !D.mesh.indices || !D.cb) return badDraw("positions, indices or cb is NULL");
        if (const std::string m = badMeshDraw(D.mesh, 1, 24, 1); !m.empty()) return badDraw(m);
        if ((uintptr_t)D.mesh.positions % 4 || (uintptr_t)D.cb % 4 || (uintptr_t)D.mesh.indices % (D.mesh.indexBits / 8))
            return badDraw("positions / cb must be 4-byte aligned, indices aligned to their size");
        if (D.mesh.numIndices) { totalTris += D.mesh.numIndices / 3; ++numJobs; }
    }
    if (totalTris >= kOutlineMaxTriangles) return fail(ctx, VQHIP_ERR_UNSUPPORTED, w + ": 2^28 or more triangles in one call");
    if (numJobs > kRasterMaxDraws) return fail(ctx, VQHIP_ERR_UNSUPPORTED, w + ": more than 20000 draws in one call");
    size_t offColors, colorCap, offBoxes, offRecords, need;
    if (!outlineLayout(totalTris, &offColors, &colorCap, &offBoxes, &offRecords, &need) || workBytes < need)
        return bad("workBytes below vqhip_outline_work_bytes(the call's triangles)");
    const void* const planes[3] = { out->sceneColor, out->selection, out->writer };
    const size_t bytes[3] = { planeExtent(width, height, pitch, 8), planeExtent(width, height, selPitch, 1), planeExtent(width, height, wrPitch, 4) };
    for (int k = 0; k < 3; ++k) {
        if (!planes[k]) continue;
        if (rangesOverlap(work, need, planes[k], bytes[k])) return bad("an output overlaps the work buffer");
        for (int m = 0; m < k; ++m) if (planes[m] && rangesOverlap(planes[m], bytes[m], planes[k], bytes[k])) return bad("an output overlaps another output");
    }

    OutlineArgs a;
    std::memset(&a, 0, sizeof(a));
    a.sceneColor = out->sceneColor; a.selection = out->selection; a.writer = out->writer;
    a.colors = (OutlineColor*)((char*)work + offColors); a.colorCap = (uint32_t)colorCap;
    a.recCap = totalTris * kOutlineFanMax; a.pitch = (uint32_t)pitch; a.selectionPitch = (uint32_t)selPitch; a.writerPitch = (uint32_t)wrPitch;
    a.width = width; a.height = height;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    uint32_t* counter = (uint32_t*)work;
    void* boxes = (char*)work + offBoxes;
    void* records = (char*)work + offRecords;
    hipError_t e = launch_raster_begin(st, counter, 1);
    if (e != hipSuccess) return failHip(ctx, e, (w + " counter launch").c_str());
    // the draws that have indices, in ring slots of OutlineJobs: one setup launch per slot
    int d = 0;
    uint64_t blocks = 0;
    auto fill = [&](OutlineJob& J, size_t k) {
        if (!k) blocks = 0;
        while (!draws[d].mesh.numIndices) ++d;
        const vqhip_outline_draw& D = draws[d];
        std::memset(&J, 0, sizeof(J));
        J.positions = (const uint8_t*)D.mesh.positions; J.indices = D.mesh.indices; J.cb = D.cb;
        J.strideBytes = D.mesh.strideBytes; J.numVertices = D.mesh.numVertices; J.numTris = D.mesh.numIndices / 3; J.indexBits = D.mesh.indexBits;
        J.firstBlock = (uint32_t)blocks; J.drawIndex = (uint32_t)d;
        blocks += ((uint64_t)J.numTris + 255) / 256;
        ++d;
    };
    auto setup = [&](const OutlineJob* jobs, size_t n, size_t first) {
        hipError_t le = launch_outline_setup(st, jobs, (int)n, (uint32_t)first, (uint32_t)blocks, a, counter, boxes, records);
        return le == hipSuccess ? VQHIP_OK : failHip(ctx, le, (w + " setup launch").c_str());
    };
    if (int rc = stageJobs<OutlineJob>(ctx, st, numJobs, fill, setup)) return rc;
    e = launch_outline_fill(st, a, ctx->opt.rasterTile == 64 ? 64 : 32, counter, boxes, records);
    return e == hipSuccess ? VQHIP_OK : failHip(ctx, e, (w + " fill launch").c_str());
}

// ---- Unlit draws (raster_unlit.hip; docs/DESIGN_DETAILS.md §7.23 U1 .. U7) -------------------------------------------------------------------------------------------
static_assert(slotsFor<UnlitJob>(kRasterMaxDraws) < vqhip_ctx::kSlots, "one call never laps the ring");
static constexpr uint64_t kUnlitMaxTriangles = (uint64_t)1 << 28;     // eight slots each: a slot number is 32 bits wide
// UnlitColor[min(triangles, max draws), at least 1] | triangle boxes[n] | boxes[8 n] | records[8 n]; false above the limit or when the sizes do not fit
static bool unlitLayout(uint64_t triangles, size_t* colorCap, size_t* triBoxes, size_t* boxes, size_t* records, size_t* total) {
    if (triangles >= kUnlitMaxTriangles) return false;
    const uint64_t cap = triangles * kUnlitFanMax, nc = triangles < kRasterMaxDraws ? (triangles ? triangles : 1) : kRasterMaxDraws;
    const uint64_t tb = align256(nc * sizeof(UnlitColor)), b = align256(tb + triangles * kUnlitBoxBytes), r = align256(b + cap * kUnlitBoxBytes),
                   t = align256(r + cap * kUnlitRecordBytes);
    if (t > (uint64_t)SIZE_MAX) return false;
    *colorCap = (size_t)nc; *triBoxes = (size_t)tb; *boxes = (size_t)b; *records = (size_t)r; *total = (size_t)t;
    return true;
}

size_t vqhip_unlit_draws_work_bytes(uint64_t triangles) {
    size_t nc, tb, b, r, t;
    return unlitLayout(triangles, &nc, &tb, &b, &r, &t) ? t : 0;
}

int vqhip_unlit_draws(vqhip_ctx* ctx, void* stream, const vqhip_unlit_draw* draws, int numDraws, int width, int height, int blend,
                      const vqhip_unlit_targets* out, void* work, size_t workBytes) {
    if (!ctx) return fail(nullptr, VQHIP_ERR_INVALID_ARG, "unlit_draws: ctx is NULL");
    CTX_GUARD(ctx, "unlit_draws");
    vqk::Range range_("RenderUnlitDraws");
    const std::string w = "unlit_draws";
    auto bad = [&](const std::string& m) { return fail(ctx, VQHIP_ERR_INVALID_ARG, w + ": " + m); };
    if (!out || !out->sceneColor || !out->sceneDepth || !work) return bad("NULL argument (out, out->sceneColor, out->sceneDepth or work)");
    if (numDraws < 0 || (numDraws > 0 && !draws)) return bad("numDraws < 0, or draws is NULL");
    if (width < 1 || width > VQHIP_SCENE_DEPTH_MAX_DIM || height < 1 || height > VQHIP_SCENE_DEPTH_MAX_DIM) return bad("width and height must be 1..8192");
    if (blend != 0 && blend != 1) return bad("blend must be 0 or 1");
    if (out->reserved != 0) return bad("reserved must be 0");
    if (out->pitch < 0 || out->depth_pitch < 0 || out->writer_pitch < 0) return bad("negative pitch");
    const size_t pitch = out->pitch ? (size_t)out->pitch : (size_t)width, zPitch = out->depth_pitch ? (size_t)out->depth_pitch : (size_t)width;
    const size_t wrPitch = out->writer_pitch ? (size_t)out->writer_pitch : (size_t)width;
    if (pitch < (size_t)width || zPitch < (size_t)width || wrPitch < (size_t)width) return bad("a pitch below width");
    if ((uintptr_t)out->sceneColor % 8) return bad("sceneColor is not 8-byte aligned");
    if ((uintptr_t)out->sceneDepth % 4) return bad("sceneDepth must be 4-byte aligned");
    if ((uintptr_t)out->writer % 4) return bad("writer must be 4-byte aligned");
    if ((uintptr_t)work % 256) return bad("work must be 256-byte aligned");
    uint64_t totalTris = 0;
    size_t numJobs = 0;
    for (int d = 0; d < numDraws; ++d) {
        const vqhip_unlit_draw& D = draws[d];
        auto badDraw = [&](const std::string& m) { return bad("draw " + std::to_string(d) + ": " + m); };
        if (!D.mesh.positions || !D.mesh.indices || !D.cb) return badDraw("positions, indices or cb is NULL");
        if (const std::string m = badMeshDraw(D.mesh, 1, 12, 1); !m.empty()) return badDraw(m);
        if (D.cullMode != VQHIP_CULL_NONE && D.cullMode != VQHIP_CULL_FRONT && D.cullMode != VQHIP_CULL_BACK) return badDraw("unknown cullMode");
        if (D.reserved != 0) return badDraw("reserved must be 0");
        if ((uintptr_t)D.mesh.positions % 4 || (uintptr_t)D.cb % 4 || (uintptr_t)D.mesh.indices % (D.mesh.indexBits / 8))
            return badDraw("positions / cb must be 4-byte aligned, indices aligned to their size");
        if (D.mesh.numIndices) { totalTris += D.mesh.numIndices / 3; ++numJobs; }
    }
    if (totalTris >= kUnlitMaxTriangles) return fail(ctx, VQHIP_ERR_UNSUPPORTED, w + ": 2^28 or more triangles in one call");
    if (numJobs > kRasterMaxDraws) return fail(ctx, VQHIP_ERR_UNSUPPORTED, w + ": more than 20000 draws in one call");
    size_t colorCap, offTriBoxes, offBoxes, offRecords, need;
    if (!unlitLayout(totalTris, &colorCap, &offTriBoxes, &offBoxes, &offRecords, &need) || workBytes < need)
        return bad("workBytes below vqhip_unlit_draws_work_bytes(the call's triangles)");
    const void* const planes[3] = { out->sceneColor, out->writer, out->sceneDepth };        // the input last: it must not overlap an output either
    const size_t bytes[3] = { planeExtent(width, height, pitch, 8), planeExtent(width, height, wrPitch, 4), planeExtent(width, height, zPitch, 4) };
    for (int k = 0; k < 3; ++k) {
        if (!planes[k]) continue;
        if (rangesOverlap(work, need, planes[k], bytes[k])) return bad(k == 2 ? "sceneDepth overlaps the work buffer" : "an output overlaps the work buffer");
        for (int m = 0; m < k; ++m)
            if (planes[m] && rangesOverlap(planes[m], bytes[m], planes[k], bytes[k])) return bad(k == 2 ? "sceneDepth overlaps an output" : "an output overlaps another output");
    }

    UnlitArgs a;
    std::memset(&a, 0, sizeof(a));
    a.sceneColor = out->sceneColor; a.sceneDepth = out->sceneDepth; a.writer = out->writer;
    a.colors = (UnlitColor*)work; a.colorCap = (uint32_t)colorCap;
    a.slots = (uint32_t)(totalTris * kUnlitFanMax); a.pitch = (uint32_t)pitch; a.depthPitch = (uint32_t)zPitch; a.writerPitch = (uint32_t)wrPitch;
    a.width = width; a.height = height; a.blend = blend;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    void* triBoxes = (char*)work + offTriBoxes;
    void* boxes = (char*)work + offBoxes;
    void* records = (char*)work + offRecords;
    // the draws that have indices, in ring slots of UnlitJobs: one setup launch per slot
    int d = 0;
    uint64_t blocks = 0, firstQ = 0;
    auto fill = [&](UnlitJob& J, size_t k) {
        if (!k) blocks = 0;
        while (!draws[d].mesh.numIndices) ++d;
        const vqhip_unlit_draw& D = draws[d];
        std::memset(&J, 0, sizeof(J));
        J.positions = (const uint8_t*)D.mesh.positions; J.indices = D.mesh.indices; J.cb = D.cb;
        J.strideBytes = D.mesh.strideBytes; J.numVertices = D.mesh.numVertices; J.numTris = D.mesh.numIndices / 3; J.indexBits = D.mesh.indexBits;
        J.firstBlock = (uint32_t)blocks; J.drawIndex = (uint32_t)d; J.firstQ = (uint32_t)firstQ; J.cullMode = D.cullMode;
        blocks += ((uint64_t)J.numTris + 255) / 256;
        firstQ += J.numTris;
        ++d;
    };
    auto setup = [&](const UnlitJob* jobs, size_t n, size_t first) {
        hipError_t le = launch_unlit_setup(st, jobs, (int)n, (uint32_t)first, (uint32_t)blocks, a, triBoxes, boxes, records);
        return le == hipSuccess ? VQHIP_OK : failHip(ctx, le, (w + " setup launch").c_str());
    };
    if (int rc = stageJobs<UnlitJob>(ctx, st, numJobs, fill, setup)) return rc;
    if (!a.slots && !a.writer) return VQHIP_OK;                     // no fragment, no plane to clear
    hipError_t e = launch_unlit_fill(st, a, ctx->opt.rasterTile == 64 ? 64 : 32, triBoxes, boxes, records);
    return e == hipSuccess ? VQHIP_OK : failHip(ctx, e, (w + " fill launch").c_str());
}

// ---- Line draws (raster_lines.hip; docs/DESIGN_DETAILS.md §7.24 L1 .. L8) --------------------------------------------------------------------------------------------
static_assert(slotsFor<LineJob>(kRasterMaxDraws) < vqhip_ctx::kSlots, "one call never laps the ring");
static constexpr uint64_t kLinesMax = (uint64_t)1 << 31;             // the fill's LDS word holds q + 1 in 32 bits, and a block number stays far below 2^31
// LineColor[4 x min(lines, max draws), at least 4] | boxes[n] | records[n]; false above the limit or when the sizes do not fit
static bool linesLayout(uint64_t lines, size_t* colorCap, size_t* boxes, size_t* records, size_t* total) {
    if (lines >= kLinesMax) return false;
    const uint64_t nc = (lines < kRasterMaxDraws ? (lines ? lines : 1) : kRasterMaxDraws) * kLineColorsPerJob;
    const uint64_t b = align256(nc * sizeof(LineColor)), r = align256(b + lines * kLineBoxBytes), t = align256(r + lines * kLineRecordBytes);
    if (t > (uint64_t)SIZE_MAX) return false;
    *colorCap = (size_t)nc; *boxes = (size_t)b; *records = (size_t)r; *total = (size_t)t;
    return true;
}

size_t vqhip_line_draws_work_bytes(uint64_t lines) {
    size_t nc, b, r, t;
    return linesLayout(lines, &nc, &b, &r, &t) ? t : 0;
}

int vqhip_line_draws(vqhip_ctx* ctx, void* stream, const vqhip_line_draw* draws, int numDraws, int width, int height, const vqhip_unlit_targets* out, void* work,
                     size_t workBytes) {
    if (!ctx) return fail(nullptr, VQHIP_ERR_INVALID_ARG, "line_draws: ctx is NULL");
    CTX_GUARD(ctx, "line_draws");
    vqk::Range range_("RenderLineDraws");
    const std::string w = "line_draws";
    auto bad = [&](const std::string& m) { return fail(ctx, VQHIP_ERR_INVALID_ARG, w + ": " + m); };
    if (!out || !out->sceneColor || !out->sceneDepth || !work) return bad("NULL argument (out, out->sceneColor, out->sceneDepth or work)");
    if (numDraws < 0 || (numDraws > 0 && !draws)) return bad("numDraws < 0, or draws is NULL");
    if (width < 1 || width > VQHIP_SCENE_DEPTH_MAX_DIM || height < 1 || height > VQHIP_SCENE_DEPTH_MAX_DIM) return bad("width and height must be 1..8192");
    if (out->reserved != 0) return bad("reserved must be 0");
    if (out->pitch < 0 || out->depth_pitch < 0 || out->writer_pitch < 0) return bad("negative pitch");
    const size_t pitch = out->pitch ? (size_t)out->pitch : (size_t)width, zPitch = out->depth_pitch ? (size_t)out->depth_pitch : (size_t)width;
    const size_t wrPitch = out->writer_pitch ? (size_t)out->writer_pitch : (size_t)width;
    if (pitch < (size_t)width || zPitch < (size_t)width || wrPitch < (size_t)width) return bad("a pitch below width");
    if ((uintptr_t)out->sceneColor % 8) return bad("sceneColor is not 8-byte aligned");
    if ((uintptr_t)out->sceneDepth % 4) return bad("sceneDepth must be 4-byte aligned");
    if ((uintptr_t)out->writer % 4) return bad("writer must be 4-byte aligned");
    if ((uintptr_t)work % 256) return bad("work must be 256-byte aligned");
    auto linesOf = [](const vqhip_line_draw& D) {
        return D.kind == VQHIP_LINES_WIREFRAME ? (uint64_t)D.mesh.numIndices * D.numInstances : (uint64_t)D.mesh.numIndices * 3;
    };
    uint64_t totalLines = 0;
    size_t numJobs = 0;
    for (int d = 0; d < numDraws; ++d) {
        const vqhip_line_draw& D = draws[d];
        auto badDraw = [&](const std::string& m) { return bad("draw " + std::to_string(d) + ": " + m); };
        if (D.kind != VQHIP_LINES_WIREFRAME && D.kind != VQHIP_LINES_VERTEX_AXES) return badDraw("unknown kind");
        const bool wire = D.kind == VQHIP_LINES_WIREFRAME;
        if (!D.mesh.positions || !D.mesh.indices) return badDraw("positions or indices is NULL");
        if (wire ? (!D.matModelViewProj || !D.color || D.axes) : (!D.axes || D.matModelViewProj || D.color))
            return badDraw(wire ? "WIREFRAME takes matModelViewProj and color, and axes NULL" : "VERTEX_AXES takes axes, and matModelViewProj and color NULL");
        if (D.mesh.indexBits != 16 && D.mesh.indexBits != 32) return badDraw("indexBits must be 16 or 32");
        if (wire) {
            if (const std::string m = badMeshDraw(D.mesh, D.numInstances, 12, VQHIP_LINES_MAX_INSTANCES); !m.empty()) return badDraw(m);
        } else {
            if (D.mesh.strideBytes < 36 || D.mesh.strideBytes % 4) return badDraw("strideBytes below 36 or not a multiple of 4");
            if (D.numInstances != 1) return badDraw("numInstances must be 1");
        }
        if ((uintptr_t)D.mesh.positions % 4 || (uintptr_t)D.matModelViewProj % 4 || (uintptr_t)D.color % 4 || (uintptr_t)D.axes % 4 ||
            (uintptr_t)D.mesh.indices % (D.mesh.indexBits / 8))
            return badDraw("positions / matModelViewProj / color / axes must be 4-byte aligned, indices aligned to their size");
        if (D.mesh.numIndices) { totalLines += linesOf(D); ++numJobs; }
    }
    if (totalLines >= kLinesMax) return fail(ctx, VQHIP_ERR_UNSUPPORTED, w + ": 2^31 or more lines in one call");
    if (numJobs > kRasterMaxDraws) return fail(ctx, VQHIP_ERR_UNSUPPORTED, w + ": more than 20000 draws in one call");
    size_t colorCap, offBoxes, offRecords, need;
    if (!linesLayout(totalLines, &colorCap, &offBoxes, &offRecords, &need) || workBytes < need)
        return bad("workBytes below vqhip_line_draws_work_bytes(the call's lines)");
    const void* const planes[3] = { out->sceneColor, out->writer, out->sceneDepth };        // the input last: it must not overlap an output either
    const size_t bytes[3] = { planeExtent(width, height, pitch, 8), planeExtent(width, height, wrPitch, 4), planeExtent(width, height, zPitch, 4) };
    for (int k = 0; k < 3; ++k) {
        if (!planes[k]) continue;
        if (rangesOverlap(work, need, planes[k], bytes[k])) return bad(k == 2 ? "sceneDepth overlaps the work buffer" : "an output overlaps the work buffer");
        for (int m = 0; m < k; ++m)
            if (planes[m] && rangesOverlap(planes[m], bytes[m], planes[k], bytes[k])) return bad(k == 2 ? "sceneDepth overlaps an output" : "an output overlaps another output");
    }

    LineArgs a;
    std::memset(&a, 0, sizeof(a));
    a.sceneColor = out->sceneColor; a.sceneDepth = out->sceneDepth; a.writer = out->writer;
    a.colors = (LineColor*)work; a.colorCap = (uint32_t)colorCap;
    a.lines = (uint32_t)totalLines; a.pitch = (uint32_t)pitch; a.depthPitch = (uint32_t)zPitch; a.writerPitch = (uint32_t)wrPitch;
    a.width = width; a.height = height;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    void* boxes = (char*)work + offBoxes;
    void* records = (char*)work + offRecords;
    // the draws that have indices, in ring slots of LineJobs: one setup launch per slot
    int d = 0;
    uint64_t blocks = 0, firstQ = 0;
    auto fill = [&](LineJob& J, size_t k) {
        if (!k) blocks = 0;
        while (!draws[d].mesh.numIndices) ++d;
        const vqhip_line_draw& D = draws[d];
        std::memset(&J, 0, sizeof(J));
        const bool wire = D.kind == VQHIP_LINES_WIREFRAME;
        J.vertices = (const uint8_t*)D.mesh.positions; J.indices = D.mesh.indices; J.color = D.color;
        J.cb = wire ? (const void*)D.matModelViewProj : (const void*)D.axes;
        J.strideBytes = D.mesh.strideBytes; J.numVertices = D.mesh.numVertices; J.numPrims = wire ? D.mesh.numIndices / 3 : D.mesh.numIndices;
        J.numLines = (uint32_t)linesOf(D); J.indexBits = (uint16_t)D.mesh.indexBits; J.kind = (uint16_t)D.kind;
        J.firstBlock = (uint32_t)blocks; J.drawIndex = (uint32_t)d; J.firstQ = (uint32_t)firstQ;
        blocks += ((uint64_t)J.numLines + 255) / 256;
        firstQ += J.numLines;
        ++d;
    };
    auto setup = [&](const LineJob* jobs, size_t n, size_t first) {
        hipError_t le = launch_lines_setup(st, jobs, (int)n, (uint32_t)first, (uint32_t)blocks, a, boxes, records);
        return le == hipSuccess ? VQHIP_OK : failHip(ctx, le, (w + " setup launch").c_str());
    };
    if (int rc = stageJobs<LineJob>(ctx, st, numJobs, fill, setup)) return rc;
    if (!a.lines && !a.writer) return VQHIP_OK;                     // no fragment, no plane to clear
    hipError_t e = launch_lines_fill(st, a, ctx->opt.rasterTile == 64 ? 64 : 32, boxes, records);
    return e == hipSuccess ? VQHIP_OK : failHip(ctx, e, (w + " fill launch").c_str());
}

// ---- Heightmap displacement of vertex streams (displace.hip; docs/DESIGN_DETAILS.md §7.22 H1 .. H4) -------------------------------------------------------------------
static_assert((vqhip_ctx::kSlots - 1) * (kConstSlotBytes / sizeof(DisplaceJob)) == VQHIP_DISPLACE_MAX_JOBS, "VQHIP_DISPLACE_MAX_JOBS is what 31 ring slots hold");
static_assert(slotsFor<DisplaceJob>(VQHIP_DISPLACE_MAX_JOBS) < vqhip_ctx::kSlots, "one call never laps the ring");

int vqhip_displace_meshes(vqhip_ctx* ctx, void* stream, const vqhip_displace_job* jobs, int numJobs) {
    if (!ctx) return fail(nullptr, VQHIP_ERR_INVALID_ARG, "displace_meshes: ctx is NULL");
    CTX_GUARD(ctx, "displace_meshes");
    vqk::Range range_("DisplaceMeshes");
    const std::string w = "displace_meshes";
    auto bad = [&](const std::string& m) { return fail(ctx, VQHIP_ERR_INVALID_ARG, w + ": " + m); };
    if (numJobs < 0 || (numJobs > 0 && !jobs)) return bad("numJobs < 0, or jobs is NULL");
    uint64_t totalVertices = 0;
    size_t numLive = 0;
    // what a job reads and writes: [3 j] its input, [3 j + 1] its height map's chain, [3 j + 2] its output; p NULL (a job without vertices, the null SRV): nothing
    std::vector<Span> spans((size_t)numJobs * 3, Span{ nullptr, 0, "" });
    for (int j = 0; j < numJobs; ++j) {
        const vqhip_displace_job& J = jobs[j];
        auto badJob = [&](const std::string& m) { return bad("job " + std::to_string(j) + ": " + m); };
        if (J.numVertices && (!J.vertices || !J.out)) return badJob("vertices or out is NULL");
        if (J.strideBytes < 44 || J.strideBytes > 2048 || J.strideBytes % 4) return badJob("strideBytes must be 44..2048 and a multiple of 4");
        if (J.outStrideBytes != 12 && J.outStrideBytes != J.strideBytes) return badJob("outStrideBytes must be 12 or strideBytes");
        if (J.reserved != 0) return badJob("reserved must be 0");
        if ((uintptr_t)J.vertices % 4 || (uintptr_t)J.out % 4) return badJob("vertices / out must be 4-byte aligned");
        if (J.heightmap.texels) {                             // a null SRV samples 0: its dimensions are not read
            const vqhip_texture2d& t = J.heightmap;
            if (t.width < 1 || t.width > VQHIP_MASK_TEXTURE_MAX_DIM || t.height < 1 || t.height > VQHIP_MASK_TEXTURE_MAX_DIM) return badJob("height map: width and height must be 1..16384");
            if (t.mips < 1 || t.mips > vqhip_mip_level_count(t.width, t.height)) return badJob("height map: mips must be 1..vqhip_mip_level_count(width, height)");
            if ((uintptr_t)t.texels % 4) return badJob("height map: texels must be 4-byte aligned");
        }
        if (!J.numVertices) continue;
        totalVertices += J.numVertices; ++numLive;
        spans[3 * (size_t)j] = { J.vertices, planeExtent((int)J.strideBytes, (int)J.numVertices, J.strideBytes, 1), "input" };
        if (J.heightmap.texels) spans[3 * (size_t)j + 1] = { J.heightmap.texels, vqhip_mip_chain_bytes_rgba8(J.heightmap.width, J.heightmap.height, J.heightmap.mips), "height map" };
        spans[3 * (size_t)j + 2] = { J.out, planeExtent((int)J.outStrideBytes, (int)J.numVertices, J.outStrideBytes, 1), "output" };
    }
    if (totalVertices >= ((uint64_t)1 << 31)) return fail(ctx, VQHIP_ERR_UNSUPPORTED, w + ": 2^31 or more vertices in one call");
    if (numLive > VQHIP_DISPLACE_MAX_JOBS) return fail(ctx, VQHIP_ERR_UNSUPPORTED, w + ": more than " + std::to_string(VQHIP_DISPLACE_MAX_JOBS) + " jobs with vertices in one call");
    // An output must not meet anything else the call touches. In the order of their first bytes, a span overlaps an earlier one iff it starts before the
    // furthest end seen so far: one sorted sweep keeps the furthest end of the outputs and of everything, instead of comparing every pair of up to 17 236 jobs.
    {
        std::vector<uint32_t> order;
        for (size_t k = 0; k < spans.size(); ++k) if (spans[k].p && spans[k].n) order.push_back((uint32_t)k);
        std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return (uintptr_t)spans[a].p < (uintptr_t)spans[b].p; });
        int lastOut = -1, lastAny = -1;                       // the spans whose ends reach furthest so far
        auto end = [&](int k) { return (uintptr_t)spans[(size_t)k].p + spans[(size_t)k].n; };
        for (uint32_t k : order) {
            const Span& s = spans[k];
            const bool isOut = k % 3 == 2;
            const int hit = lastOut >= 0 && rangesOverlap(s.p, s.n, spans[(size_t)lastOut].p, spans[(size_t)lastOut].n) ? lastOut
                          : isOut && lastAny >= 0 && rangesOverlap(s.p, s.n, spans[(size_t)lastAny].p, spans[(size_t)lastAny].n) ? lastAny : -1;
            if (hit >= 0) {
                const int o = isOut ? (int)k : hit, other = isOut ? hit : (int)k;
                return bad("job " + std::to_string(o / 3) + ": the output overlaps the " + spans[(size_t)other].name + " of job " + std::to_string(other / 3) +
                           (o / 3 == other / 3 && other % 3 == 0 ? " (displacing in place is refused: a second call would displace twice)" : ""));
            }
            if (isOut && (lastOut < 0 || end((int)k) > end(lastOut))) lastOut = (int)k;
            if (lastAny < 0 || end((int)k) > end(lastAny)) lastAny = (int)k;
        }
    }
    if (!numLive) return VQHIP_OK;

    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    // the jobs that have vertices, in ring slots of DisplaceJobs: one launch per slot
    int j = 0;
    uint64_t blocks = 0;
    auto fill = [&](DisplaceJob& D, size_t k) {
        if (!k) blocks = 0;
        while (!jobs[j].numVertices) ++j;
        const vqhip_displace_job& J = jobs[j++];
        std::memset(&D, 0, sizeof(D));
        D.vertices = J.vertices; D.out = J.out; D.texels = J.heightmap.texels;
        D.strideBytes = J.strideBytes; D.outStrideBytes = J.outStrideBytes; D.numVertices = J.numVertices;
        D.width = J.heightmap.width; D.height = J.heightmap.height;
        D.sx = J.uvScaleOffset.x; D.sy = J.uvScaleOffset.y; D.ox = J.uvScaleOffset.z; D.oy = J.uvScaleOffset.w;
        D.displacement = J.displacement;
        D.firstBlock = (uint32_t)blocks;                      // below 2^23 + the slot's jobs: the call has fewer than 2^31 vertices
        blocks += ((uint64_t)J.numVertices + kDisplaceLanes - 1) / kDisplaceLanes;
    };
    auto launch = [&](const DisplaceJob* slotJobs, size_t n, size_t) {
        hipError_t le = launch_displace(st, slotJobs, (int)n, (uint32_t)blocks);
        return le == hipSuccess ? VQHIP_OK : failHip(ctx, le, (w + " launch").c_str());
    };
    return stageJobs<DisplaceJob>(ctx, st, numLive, fill, launch);
}

} // extern "C"

