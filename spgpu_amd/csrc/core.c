/*
 * Handle / runtime layer of the spgpu-amd C ABI (include/spgpu/core.h).
 * Behavioural model: reference src/core/core.c:11-99.  Written for HIP on
 * MI355X; the handle additionally owns the scratch that the reductions use
 * (the reference keeps that in a process-global __device__ array,
 * kernels/ddot.cu:35).
 */
#include "spgpu_internal.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

/* ---- deep lists of the ELL/HELL SpMV (spgpu_internal.h): one per stream ---- */
#define DEEP_HEAD_BYTES (SPGPU_DEEP_HEAD_INTS * sizeof(int))
#define DEEP_ENTRY_BYTES ((size_t)SPGPU_DEEP_ENTRIES * sizeof(SpgpuDeepEntry))
#define DEEP_ITEM_ENTRY_BYTES ((size_t)SPGPU_DEEP_ITEMS * sizeof(SpgpuDeepItem))
#define DEEP_PARTIAL_BYTES ((size_t)SPGPU_DEEP_ENTRIES * 32 * 16)
#define DEEP_ITEM_SUM_BYTES ((size_t)SPGPU_DEEP_ITEMS * 32 * 16)

/* Gives `stream` a list if it has none and the table has room (device already current).  Allocates and clears with a
 * blocking call: this runs in spgpuCreate / spgpuSetStream, outside any launch path and outside any stream capture. */
static void deepListFor(SpgpuPrivateHandle* h, hipStream_t stream)
{
    pthread_mutex_lock(&h->tablesLock);
    int known = 0;
    for (int i = 0; i < h->deepStreams; ++i)
        known |= h->deepStream[i] == stream;
    if (!known && h->deepStreams < SPGPU_DEEP_STREAMS) {
        void* p = NULL;
        hipEvent_t idle = NULL;
        if (hipMalloc(&p, DEEP_HEAD_BYTES + DEEP_ENTRY_BYTES + DEEP_ITEM_ENTRY_BYTES + DEEP_PARTIAL_BYTES + DEEP_ITEM_SUM_BYTES) == hipSuccess) {
            if (spgpuTuning()->poisonScratch)
                (void)hipMemset((char*)p + DEEP_HEAD_BYTES + DEEP_ENTRY_BYTES + DEEP_ITEM_ENTRY_BYTES, 0xFF, DEEP_PARTIAL_BYTES + DEEP_ITEM_SUM_BYTES);
            if (hipMemset(p, 0, DEEP_HEAD_BYTES + DEEP_ENTRY_BYTES + DEEP_ITEM_ENTRY_BYTES) == hipSuccess &&
                hipEventCreateWithFlags(&idle, hipEventDisableTiming) == hipSuccess) {
                h->deepScratch[h->deepStreams] = p;
                h->deepStream[h->deepStreams] = stream;
                h->deepIdle[h->deepStreams] = idle;
                h->deepUsed[h->deepStreams] = 0;
                h->deepPinned[h->deepStreams] = 0;
                h->deepClock[h->deepStreams] = ++h->deepTick;
                h->deepStreams += 1;
            } else {
                hipFree(p);
            }
        }
    } else if (!known) {
        /* Every list has an owner.  A program that creates and destroys streams as it goes would fill the table with
         * the lists of streams that no longer exist, and every ordered SpMV on a later stream would run the kernel that
         * needs no list for good (slower, another order of additions).  So the list that was used longest ago AND whose
         * last user has finished -- the event recorded behind its deep kernels has completed, or it was never used --
         * changes hands: its header is zero (the last finishing workgroup of a call leaves it so), nothing else of it
         * carries over from call to call. */
        int pick = -1;
        for (int i = 0; i < h->deepStreams; ++i) {
            if (h->deepStream[i] == h->pub.defaultStream || h->deepPinned[i])
                continue; /* the default stream always comes back (spgpuSetStream(h, 0)); a captured graph may replay at any time */
            if (h->deepUsed[i] && !spgpuEventDone(h->deepIdle[i]))
                continue;
            if (pick < 0 || h->deepClock[i] < h->deepClock[pick])
                pick = i;
        }
        if (pick >= 0) {
            h->deepStream[pick] = stream;
            h->deepUsed[pick] = 0;
            h->deepClock[pick] = ++h->deepTick;
            h->deepRecycled += 1;
        }
    }
    pthread_mutex_unlock(&h->tablesLock);
}

spgpuStatus_t spgpuCreate(spgpuHandle_t* pHandle, int device)
{
    if (!pHandle)
        return SPGPU_UNSPECIFIED;
    *pHandle = NULL;

    hipDeviceProp_t prop;
    hipError_t perr = hipGetDeviceProperties(&prop, device);
    if (perr != hipSuccess) {
        fprintf(stderr, "spgpuCreate: hipGetDeviceProperties(%d) failed: %s\n", device, hipGetErrorString(perr));
        return SPGPU_UNSPECIFIED;
    }

    SpgpuPrivateHandle* h = (SpgpuPrivateHandle*)calloc(1, sizeof(SpgpuPrivateHandle));
    if (!h)
        return SPGPU_OUTOFMEMORY;

    int previous = 0;
    hipGetDevice(&previous);
    hipError_t err = hipSetDevice(device);
    if (err == hipSuccess)
        err = hipStreamCreate(&h->pub.defaultStream);
    if (err == hipSuccess)
        err = hipMalloc(&h->reduceScratch, SPGPU_REDUCE_SCRATCH_BYTES);
    if (err == hipSuccess && spgpuTuning()->poisonScratch)
        err = hipMemset(h->reduceScratch, 0xFF, SPGPU_REDUCE_SCRATCH_BYTES);
    if (err == hipSuccess)
        err = hipHostMalloc(&h->reduceHost, SPGPU_REDUCE_SCRATCH_BYTES, hipHostMallocDefault);
    if (err == hipSuccess)
        err = hipHostMalloc((void**)&h->formFeedback, (SPGPU_FEEDBACK_ENTRIES + 2) * SPGPU_FEEDBACK_SAMPLES * sizeof(int),
                            hipHostMallocDefault);
    if (err == hipSuccess)
        memset(h->formFeedback, 0, (SPGPU_FEEDBACK_ENTRIES + 2) * SPGPU_FEEDBACK_SAMPLES * sizeof(int));
    hipSetDevice(previous);

    if (err != hipSuccess) {
        fprintf(stderr, "spgpuCreate: device %d setup failed: %s\n", device, hipGetErrorString(err));
        if (h->reduceScratch) hipFree(h->reduceScratch);
        if (h->reduceHost) hipHostFree(h->reduceHost);
        if (h->pub.defaultStream) hipStreamDestroy(h->pub.defaultStream);
        free(h);
        return err == hipErrorOutOfMemory ? SPGPU_OUTOFMEMORY : SPGPU_UNSPECIFIED;
    }

    h->pub.currentStream = h->pub.defaultStream;
    h->pub.device = device;
    h->pub.warpSize = prop.warpSize;
    h->pub.maxThreadsPerBlock = prop.maxThreadsPerBlock;
    h->pub.maxGridSizeX = prop.maxGridSize[0];
    h->pub.maxGridSizeY = prop.maxGridSize[1];
    h->pub.maxGridSizeZ = prop.maxGridSize[2];
    h->pub.multiProcessorCount = prop.multiProcessorCount;
    h->pub.capabilityMajor = prop.major;
    h->pub.capabilityMinor = prop.minor;
    h->magic = SPGPU_HANDLE_MAGIC;
    pthread_mutex_init(&h->tablesLock, NULL);
    h->spmvForm = SPGPU_SPMV_FORM_AUTO;
    hipSetDevice(device);
    deepListFor(h, h->pub.defaultStream); /* failing that, ordered matrices run the kernel that needs no list */
    spgpuRecordsCreate(h);
    hipSetDevice(previous);

    *pHandle = &h->pub;
    return SPGPU_SUCCESS;
}

void spgpuDestroy(spgpuHandle_t pHandle)
{
    if (!pHandle)
        return;
    SpgpuPrivateHandle* h = spgpuPrivate(pHandle);
    int previous = 0;
    hipGetDevice(&previous);
    hipSetDevice(h->pub.device);
    /* Kernels still queued on ANY stream of this device may write the pinned feedback words and read the reduction
     * scratch (a caller's stream set with spgpuSetStream, a replayed graph): wait for the whole device, not only
     * for defaultStream, before freeing them.  A graph captured from this handle must not be replayed after this. */
    hipDeviceSynchronize();
    hipFree(h->reduceScratch);
    for (int i = 0; i < h->deepStreams; ++i) {
        hipFree(h->deepScratch[i]);
        hipEventDestroy(h->deepIdle[i]);
    }
    spgpuRecordsDestroy(h);
    hipHostFree(h->reduceHost);
    hipHostFree(h->formFeedback);
    hipStreamDestroy(h->pub.defaultStream);
    hipSetDevice(previous);
    pthread_mutex_destroy(&h->tablesLock);
    h->magic = 0;
    free(h);
}

void* spgpuDeviceAlloc(spgpuHandle_t pHandle, size_t bytes)
{
    void* memory = NULL;
    int previous = 0;
    (void)hipGetDevice(&previous);
    (void)hipSetDevice(pHandle->device);
    const hipError_t allocated = hipMalloc(&memory, bytes);
    (void)hipSetDevice(previous);
    if (allocated != hipSuccess) {
        (void)hipGetLastError();
        return NULL;
    }
    return memory;
}

void spgpuStreamCreate(spgpuHandle_t pHandle, hipStream_t* stream)
{
    int previous = 0;
    hipGetDevice(&previous);
    hipSetDevice(pHandle->device);
    hipStreamCreate(stream);
    hipSetDevice(previous);
}

void spgpuStreamDestroy(hipStream_t stream)
{
    hipStreamDestroy(stream);
}

void spgpuSetStream(spgpuHandle_t pHandle, hipStream_t stream)
{
    SpgpuPrivateHandle* h = spgpuPrivate(pHandle);
    h->pub.currentStream = stream ? stream : h->pub.defaultStream;
    /* a stream the handle has not seen before gets a deep list of its own (see spgpu_internal.h): the reference's SpMV has
     * no state shared between streams (hell_spmv_base_template.cuh:336-345, core.c:64-74), so neither may this one */
    int known = 0;
    pthread_mutex_lock(&h->tablesLock);
    for (int i = 0; i < h->deepStreams; ++i)
        known |= h->deepStream[i] == h->pub.currentStream;
    pthread_mutex_unlock(&h->tablesLock);
    if (!known) {
        int previous = 0;
        hipGetDevice(&previous);
        hipSetDevice(h->pub.device);
        deepListFor(h, h->pub.currentStream);
        hipSetDevice(previous);
    }
}

hipStream_t spgpuGetStream(spgpuHandle_t pHandle)
{
    return pHandle->currentStream;
}

size_t spgpuSizeOf(spgpuType_t typeCode)
{
    switch (typeCode) {
    case SPGPU_TYPE_INT:            return sizeof(int);
    case SPGPU_TYPE_FLOAT:          return sizeof(float);
    case SPGPU_TYPE_DOUBLE:         return sizeof(double);
    case SPGPU_TYPE_COMPLEX_FLOAT:  return sizeof(hipFloatComplex);
    case SPGPU_TYPE_COMPLEX_DOUBLE: return sizeof(hipDoubleComplex);
    default:                        return 0;
    }
}

spgpuStatus_t spgpuDeepScratch(spgpuHandle_t pHandle, SpgpuDeepList* list)
{
    SpgpuPrivateHandle* h = spgpuPrivate(pHandle);
    char* base = NULL;
    pthread_mutex_lock(&h->tablesLock);
    for (int i = 0; i < h->deepStreams; ++i)
        if (h->deepStream[i] == h->pub.currentStream) {
            base = (char*)h->deepScratch[i];
            list->idle = h->deepIdle[i];
            h->deepUsed[i] = 1;
            h->deepClock[i] = ++h->deepTick;
        }
    if (!base)
        h->deepFallbacks += 1;
    pthread_mutex_unlock(&h->tablesLock);
    if (!base)
        return SPGPU_UNSUPPORTED;
    list->header = (int*)base;
    list->entries = (SpgpuDeepEntry*)(base + DEEP_HEAD_BYTES);
    list->items = (SpgpuDeepItem*)(base + DEEP_HEAD_BYTES + DEEP_ENTRY_BYTES);
    list->partials = base + DEEP_HEAD_BYTES + DEEP_ENTRY_BYTES + DEEP_ITEM_ENTRY_BYTES;
    list->itemSums = base + DEEP_HEAD_BYTES + DEEP_ENTRY_BYTES + DEEP_ITEM_ENTRY_BYTES + DEEP_PARTIAL_BYTES;
    return SPGPU_SUCCESS;
}

void spgpuDeepListPin(spgpuHandle_t pHandle)
{
    SpgpuPrivateHandle* h = spgpuPrivate(pHandle);
    pthread_mutex_lock(&h->tablesLock);
    for (int i = 0; i < h->deepStreams; ++i)
        if (h->deepStream[i] == h->pub.currentStream)
            h->deepPinned[i] = 1;
    pthread_mutex_unlock(&h->tablesLock);
}

int* spgpuAnalyseWords(spgpuHandle_t pHandle)
{
    return spgpuPrivate(pHandle)->formFeedback + SPGPU_FEEDBACK_ENTRIES * SPGPU_FEEDBACK_SAMPLES;
}

/* Pinned words the deep kernels report into (deep_items.hip.h deepFinishKernel): [0] calls whose deep list overflowed,
 * [1] / [2] the entries / items the last such call asked for. */
int* spgpuDeepOverflowWords(spgpuHandle_t pHandle)
{
    return spgpuPrivate(pHandle)->formFeedback + (SPGPU_FEEDBACK_ENTRIES + 1) * SPGPU_FEEDBACK_SAMPLES;
}

int spgpuDeepListOverflows(spgpuHandle_t pHandle)
{
    return ((volatile int*)spgpuDeepOverflowWords(pHandle))[0];
}

int spgpuDeepListFallbacks(spgpuHandle_t pHandle)
{
    SpgpuPrivateHandle* h = spgpuPrivate(pHandle);
    pthread_mutex_lock(&h->tablesLock);
    const int n = h->deepFallbacks;
    pthread_mutex_unlock(&h->tablesLock);
    return n;
}

int spgpuDeepListsRecycled(spgpuHandle_t pHandle)
{
    SpgpuPrivateHandle* h = spgpuPrivate(pHandle);
    pthread_mutex_lock(&h->tablesLock);
    const int n = h->deepRecycled;
    pthread_mutex_unlock(&h->tablesLock);
    return n;
}

/* ---- per-handle kernel-form hint (include/spgpu/tuning.h) ---- */
void spgpuSetSpmvForm(spgpuHandle_t pHandle, int form)
{
    if (form < SPGPU_SPMV_FORM_AUTO || form > SPGPU_SPMV_FORM_SWEEP)
        form = SPGPU_SPMV_FORM_AUTO;
    __atomic_store_n(&spgpuPrivate(pHandle)->spmvForm, form, __ATOMIC_RELAXED);
}

int spgpuGetSpmvForm(spgpuHandle_t pHandle)
{
    return __atomic_load_n(&spgpuPrivate(pHandle)->spmvForm, __ATOMIC_RELAXED);
}

int spgpuGetLastSpmvForm(spgpuHandle_t pHandle)
{
    return __atomic_load_n(&spgpuPrivate(pHandle)->lastSpmvForm, __ATOMIC_RELAXED);
}

void spgpuNoteSpmvForm(spgpuHandle_t pHandle, int form)
{
    __atomic_store_n(&spgpuPrivate(pHandle)->lastSpmvForm, form, __ATOMIC_RELAXED);
}

int spgpuGetLastOrderedLaunch(spgpuHandle_t pHandle)
{
    return __atomic_load_n(&spgpuPrivate(pHandle)->lastOrderedLaunch, __ATOMIC_RELAXED);
}

void spgpuNoteOrderedLaunch(spgpuHandle_t pHandle, int word)
{
    __atomic_store_n(&spgpuPrivate(pHandle)->lastOrderedLaunch, word, __ATOMIC_RELAXED);
}

/* ---- tuning knobs (include/spgpu/tuning.h) ---- */
static SpgpuTuning tuning;
static int tuningLoaded;

static int envInt(const char* name, int fallback)
{
    const char* s = getenv(name);
    return s && *s ? atoi(s) : fallback;
}

void spgpuTuningReload(void)
{
    SpgpuTuning t;
    t.xStrips = envInt("SPGPU_X_STRIPS", -1);
    t.autoSweep = envInt("SPGPU_AUTO_SWEEP", 1);
    t.poisonScratch = envInt("SPGPU_POISON_SCRATCH", 0);
    t.deepSplit = envInt("SPGPU_DEEP_SPLIT", -1);
    t.deepCap = envInt("SPGPU_DEEP_CAP", 256);
    t.deepKeep = envInt("SPGPU_DEEP_KEEP", 64);
    t.raggedShape = envInt("SPGPU_RAGGED_SHAPE", 0);
    t.raggedSplit = envInt("SPGPU_RAGGED_SPLIT", -1);
    t.plan = envInt("SPGPU_PLAN", 1);
    t.freezeEscapesPct = envInt("SPGPU_FREEZE_MAX_ESCAPES_PCT", 1);
    tuning = t;
    __atomic_store_n(&tuningLoaded, 1, __ATOMIC_RELEASE);
}

const SpgpuTuning* spgpuTuning(void)
{
    if (!__atomic_load_n(&tuningLoaded, __ATOMIC_ACQUIRE))
        spgpuTuningReload(); /* two threads racing here store the same values */
    return &tuning;
}
