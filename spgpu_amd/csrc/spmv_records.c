/* What a handle remembers about the matrices it has seen (spgpu_internal.h): AUTO's form feedback entries, the plan table with its
 * graveyard, the adopted matrices, and the holds, Thaw and byte count over them (include/spgpu/tuning.h, include/spgpu/ext/graph.h).
 * One lock guards all of it: the handle's tablesLock, which the launch paths that read a record take through spgpuTablesLock. */
#include "spgpu_internal.h"
#include "spgpu/ext/graph.h"

#include <stdlib.h>
#include <string.h>

void spgpuTablesLock(spgpuHandle_t pHandle)
{
    pthread_mutex_lock(&spgpuPrivate(pHandle)->tablesLock);
}

void spgpuTablesUnlock(spgpuHandle_t pHandle)
{
    pthread_mutex_unlock(&spgpuPrivate(pHandle)->tablesLock);
}

static void freeAdopted(const SpgpuAdopted* e)
{
    hipFree(e->values);
    hipFree(e->indices);
    hipFree(e->hackOffsetsOrdered);
    hipFree(e->lengths);
    hipFree(e->order);
}

void spgpuRecordsCreate(SpgpuPrivateHandle* h)
{
    h->adopted = (SpgpuAdopted*)calloc(SPGPU_ADOPTED, sizeof(SpgpuAdopted)); /* failing this, nothing can be adopted */
    /* the plan table (spgpu_internal.h): failing this, ordered matrices run without plans */
    h->plans = (SpgpuSpmvPlan*)calloc(SPGPU_PLANS, sizeof(SpgpuSpmvPlan));
    if (h->plans && hipHostMalloc((void**)&h->planPinned, SPGPU_PLANS * SPGPU_PLAN_WORDS * sizeof(int), hipHostMallocDefault) == hipSuccess) {
        memset(h->planPinned, 0, SPGPU_PLANS * SPGPU_PLAN_WORDS * sizeof(int));
        for (int i = 0; i < SPGPU_PLANS; ++i) {
            h->plans[i].pinned = h->planPinned + i * SPGPU_PLAN_WORDS;
            if (hipEventCreateWithFlags(&h->plans[i].built, hipEventDisableTiming) != hipSuccess)
                h->plans[i].state = SPGPU_PLAN_GIVEN_UP;
        }
    } else {
        free(h->plans);
        h->plans = NULL;
        h->planPinned = NULL;
    }
}

void spgpuRecordsDestroy(SpgpuPrivateHandle* h)
{
    if (h->adopted) {
        for (int i = 0; i < SPGPU_ADOPTED; ++i)
            if (h->adopted[i].rows > 0)
                freeAdopted(&h->adopted[i]);
        free(h->adopted);
    }
    if (h->plans) {
        for (int i = 0; i < SPGPU_PLANS; ++i) {
            if (h->plans[i].device)
                hipFree(h->plans[i].device);
            if (h->plans[i].packed)
                hipFree(h->plans[i].packed);
            if (h->plans[i].built)
                hipEventDestroy(h->plans[i].built);
        }
        free(h->plans);
    }
    for (int i = 0; i < h->planGraves; ++i)
        hipFree(h->planGraveyard[i]);
    if (h->planPinned)
        hipHostFree(h->planPinned);
}

/* ---- AUTO's form feedback: the words the sample wavefronts and probes report into, per recently seen matrix ---- */
int* spgpuFormFeedback(spgpuHandle_t pHandle, const void* key, int rows, int* calls, int* tag)
{
    /* Two host threads may share a handle (the reference documents one handle per thread, core.h:88-90, but does not
     * enforce it): the table is searched and re-assigned under a lock.  The words themselves are written by the GPU
     * and read without synchronisation by design -- any value selects a correct kernel. */
    SpgpuPrivateHandle* h = spgpuPrivate(pHandle);
    pthread_mutex_lock(&h->tablesLock);
    int* slot = NULL;
    for (unsigned e = 0; e < SPGPU_FEEDBACK_ENTRIES && !slot; ++e)
        if (h->formKey[e] == key && h->formRows[e] == rows) {
            slot = h->formFeedback + e * SPGPU_FEEDBACK_SAMPLES;
            *calls = ++h->formCalls[e];
            *tag = h->formGeneration[e] << 8;
        }
    if (!slot) {
        const unsigned e = h->formNext++ % SPGPU_FEEDBACK_ENTRIES; /* oldest entry makes room */
        h->formKey[e] = key;
        h->formRows[e] = rows;
        h->formCalls[e] = 0;
        h->formGeneration[e] = (h->formGeneration[e] + 1) & 0x7FFFFF; /* reports still in flight for the previous owner carry the old one */
        *tag = h->formGeneration[e] << 8;
        *calls = 0;
        slot = h->formFeedback + e * SPGPU_FEEDBACK_SAMPLES;
        for (int i = 0; i < SPGPU_FEEDBACK_SAMPLES; ++i)
            slot[i] = 0;
    }
    pthread_mutex_unlock(&h->tablesLock);
    return slot;
}

/* ---- per-matrix plans of the ordered ELL/HELL SpMV (spgpu_internal.h, csrc/planned_spmv.hip) ---- */
void spgpuPlanRetire(spgpuHandle_t pHandle, SpgpuSpmvPlan* plan)
{
    SpgpuPrivateHandle* h = spgpuPrivate(pHandle);
    void** const buffers[2] = {&plan->device, &plan->packed};
    for (int b = 0; b < 2; ++b) {
        if (!*buffers[b])
            continue;
        if (h->planGraves == SPGPU_PLAN_GRAVES) {
            /* kernels in flight on any stream may still read a retired plan: wait for the device before the buffers go
             * (once per SPGPU_PLAN_GRAVES retirements; never while a stream of the process captures -- see launchPlanned) */
            hipDeviceSynchronize();
            for (int i = 0; i < h->planGraves; ++i)
                hipFree(h->planGraveyard[i]);
            h->planGraves = 0;
        }
        h->planGraveyard[h->planGraves++] = *buffers[b];
        *buffers[b] = NULL;
    }
    plan->state = SPGPU_PLAN_EMPTY;
    plan->uses = 0;
    plan->deep = 0;
    plan->pinned[0] = 0;
    plan->pinned[1] = 0;
}

static int samePlanKey(const SpgpuSpmvPlan* a, const SpgpuSpmvPlan* b)
{
    return a->rP == b->rP && a->rS == b->rS && a->rIdx == b->rIdx && a->hackOffsets == b->hackOffsets &&
           a->idxStride == b->idxStride && a->rows == b->rows && a->hackSize == b->hackSize && a->baseIndex == b->baseIndex &&
           a->maxNnz == b->maxNnz && a->deepCap == b->deepCap && a->subs == b->subs;
}

SpgpuSpmvPlan* spgpuPlanRecord(spgpuHandle_t pHandle, const SpgpuSpmvPlan* key)
{
    SpgpuPrivateHandle* h = spgpuPrivate(pHandle);
    if (!h->plans)
        return NULL;
    SpgpuSpmvPlan* oldest = NULL;
    for (int i = 0; i < SPGPU_PLANS; ++i) {
        SpgpuSpmvPlan* p = &h->plans[i];
        if (p->rows > 0 && samePlanKey(p, key)) {
            p->clock = ++h->planClock;
            return p;
        }
        /* a record whose analysis is still in flight keeps its buffer and its pinned words until it has landed; a held record
         * (spgpuSpmvHold) keeps them for as long as a captured graph may replay a launch that reads them */
        if (p->holds > 0 || (p->state == SPGPU_PLAN_BUILDING && !spgpuEventDone(p->built)))
            continue;
        if (!oldest || p->rows == 0 || (oldest->rows != 0 && p->clock < oldest->clock))
            oldest = p;
    }
    if (!oldest)
        return NULL;
    const int givenUp = oldest->built == NULL; /* (its event could not be created: spgpuCreate) */
    spgpuPlanRetire(pHandle, oldest);
    int* pinned = oldest->pinned;
    hipEvent_t built = oldest->built;
    *oldest = *key;
    oldest->pinned = pinned;
    oldest->built = built;
    oldest->device = NULL;
    oldest->packed = NULL;
    oldest->state = givenUp ? SPGPU_PLAN_GIVEN_UP : SPGPU_PLAN_EMPTY;
    oldest->stales = 0;
    oldest->uses = 0;
    oldest->deep = 0;
    oldest->blocks = 0;
    oldest->holds = 0;
    oldest->clock = ++h->planClock;
    return oldest;
}

int spgpuPlanTableHeld(spgpuHandle_t pHandle)
{
    SpgpuPrivateHandle* h = spgpuPrivate(pHandle);
    int held = 0;
    if (!h->plans)
        return 0;
    pthread_mutex_lock(&h->tablesLock);
    for (int i = 0; i < SPGPU_PLANS; ++i)
        held += h->plans[i].holds > 0;
    pthread_mutex_unlock(&h->tablesLock);
    return held == SPGPU_PLANS;
}

SpgpuSpmvPlan* spgpuPlanFind(spgpuHandle_t pHandle, const SpgpuSpmvPlan* key)
{
    SpgpuPrivateHandle* h = spgpuPrivate(pHandle);
    if (!h->plans)
        return NULL;
    for (int i = 0; i < SPGPU_PLANS; ++i) {
        SpgpuSpmvPlan* p = &h->plans[i];
        if (p->rows > 0 && samePlanKey(p, key)) {
            p->clock = ++h->planClock;
            return p;
        }
    }
    return NULL;
}

void spgpuPlanCountFrozenSlabs(spgpuHandle_t pHandle)
{
    SpgpuPrivateHandle* h = spgpuPrivate(pHandle);
    h->planFrozenSlabs = 0;
    if (h->plans)
        for (int i = 0; i < SPGPU_PLANS; ++i)
            h->planFrozenSlabs += (h->plans[i].rows > 0 && h->plans[i].subs < 0 && h->plans[i].packed) ? 1 : 0;
}

int spgpuPlanLanded(SpgpuSpmvPlan* plan, int wait)
{
    if (plan->state == SPGPU_PLAN_BUILDING && (wait ? hipEventSynchronize(plan->built) == hipSuccess : spgpuEventDone(plan->built))) {
        plan->deep = ((volatile int*)plan->pinned)[0];
        plan->state = SPGPU_PLAN_READY;
    }
    return plan->state == SPGPU_PLAN_READY;
}

void spgpuSpmvPlanCounts(spgpuHandle_t pHandle, int* uses, int* builds, int* stales)
{
    SpgpuPrivateHandle* h = spgpuPrivate(pHandle);
    pthread_mutex_lock(&h->tablesLock);
    if (uses) *uses = h->planUses;
    if (builds) *builds = h->planBuilds;
    if (stales) *stales = h->planStales;
    pthread_mutex_unlock(&h->tablesLock);
}

/* ---- adopted matrices (spgpu_internal.h, csrc/adopted_hell.hip) ---- */
const SpgpuAdopted* spgpuAdoptedFind(spgpuHandle_t pHandle, hipStream_t stream, const void* cM, const int* rP, const int* rS,
                                     const int* hackOffsets, int rows, int hackSize, int baseIndex, long long valPitch, long long idxPitch)
{
    SpgpuPrivateHandle* h = spgpuPrivate(pHandle);
    if (!h->adopted || __atomic_load_n(&h->adoptedCount, __ATOMIC_RELAXED) <= 0)
        return NULL;
    /* a captured launch carries the copy's addresses for as long as the graph lives: only a held entry (spgpuSpmvHold), which Thaw
     * leaves alone, is used there */
    const int heldOnly = spgpuStreamCapturing(stream);
    const SpgpuAdopted* found = NULL;
    pthread_mutex_lock(&h->tablesLock);
    for (int i = 0; i < SPGPU_ADOPTED; ++i) {
        const SpgpuAdopted* e = &h->adopted[i];
        if (e->rows > 0 && (!heldOnly || e->holds > 0) && e->rP == (const void*)rP && e->cM == cM && e->rS == (const void*)rS && e->hackOffsets == (const void*)hackOffsets &&
            e->rows == rows && e->hackSize == hackSize && e->baseIndex == baseIndex && e->valPitch == valPitch && e->idxPitch == idxPitch) {
            found = e;
            h->adoptedUses += 1;
            break;
        }
    }
    pthread_mutex_unlock(&h->tablesLock);
    return found; /* (an entry's arrays live until spgpuSpmvThaw, which the caller may not run beside an SpMV on the same matrix) */
}

int spgpuAdoptedAdd(spgpuHandle_t pHandle, const SpgpuAdopted* entry)
{
    SpgpuPrivateHandle* h = spgpuPrivate(pHandle);
    int said = SPGPU_UNSUPPORTED;
    if (!h->adopted)
        return said;
    pthread_mutex_lock(&h->tablesLock);
    for (int i = 0; i < SPGPU_ADOPTED; ++i) {
        if (h->adopted[i].rows == 0) {
            h->adopted[i] = *entry;
            h->adoptedCount += 1;
            said = SPGPU_SUCCESS;
            break;
        }
    }
    pthread_mutex_unlock(&h->tablesLock);
    return said;
}

int spgpuAdoptedRemove(spgpuHandle_t pHandle, const int* rP, SpgpuAdopted* out)
{
    SpgpuPrivateHandle* h = spgpuPrivate(pHandle);
    int n = 0;
    if (!h->adopted)
        return 0;
    pthread_mutex_lock(&h->tablesLock);
    for (int i = 0; i < SPGPU_ADOPTED; ++i) {
        if (h->adopted[i].rows > 0 && (rP == NULL || h->adopted[i].rP == (const void*)rP)) {
            out[n++] = h->adopted[i];
            memset(&h->adopted[i], 0, sizeof(SpgpuAdopted));
            h->adoptedCount -= 1;
        }
    }
    pthread_mutex_unlock(&h->tablesLock);
    return n;
}

int spgpuSpmvAdoptedUses(spgpuHandle_t pHandle)
{
    SpgpuPrivateHandle* h = spgpuPrivate(pHandle);
    pthread_mutex_lock(&h->tablesLock);
    const int n = h->adoptedUses;
    pthread_mutex_unlock(&h->tablesLock);
    return n;
}

/* Holds on the records of the matrix with this index array (include/spgpu/ext/graph.h): its plans, its adopted entry and the plans of
 * that entry's ordered copy (keyed by the copy's indices).  delta 0: the largest count among them; +1: every READY one gains a hold
 * (none if there is no such record and no adopted entry); -1: every held one loses one.  Returns the largest count before the change. */
static int heldRecords(SpgpuPrivateHandle* h, const int* rP, int delta)
{
    int most = 0, usable = 0;
    pthread_mutex_lock(&h->tablesLock);
    SpgpuAdopted* adopted = NULL;
    for (int i = 0; h->adopted && i < SPGPU_ADOPTED; ++i)
        if (h->adopted[i].rows > 0 && h->adopted[i].rP == (const void*)rP)
            adopted = &h->adopted[i];
    const void* copy = adopted ? (const void*)adopted->indices : NULL;
    if (adopted) {
        most = adopted->holds;
        usable = 1;
    }
    for (int i = 0; i < SPGPU_PLANS; ++i) {
        SpgpuSpmvPlan* p = &h->plans[i];
        if (p->rows <= 0 || (p->rP != (const void*)rP && (!copy || p->rP != copy)))
            continue;
        most = p->holds > most ? p->holds : most;
        if (delta > 0)
            (void)spgpuPlanLanded(p, 1);
        usable += p->state == SPGPU_PLAN_READY;
    }
    if (delta > 0 && usable > 0) {
        if (adopted)
            adopted->holds += 1;
        for (int i = 0; i < SPGPU_PLANS; ++i) {
            SpgpuSpmvPlan* p = &h->plans[i];
            if (p->rows > 0 && p->state == SPGPU_PLAN_READY && (p->rP == (const void*)rP || (copy && p->rP == copy)))
                p->holds += 1;
        }
    } else if (delta > 0) {
        most = -1; /* nothing to hold */
    } else if (delta < 0 && most > 0) {
        if (adopted && adopted->holds > 0)
            adopted->holds -= 1;
        for (int i = 0; i < SPGPU_PLANS; ++i) {
            SpgpuSpmvPlan* p = &h->plans[i];
            if (p->rows > 0 && p->holds > 0 && (p->rP == (const void*)rP || (copy && p->rP == copy)))
                p->holds -= 1;
        }
    }
    pthread_mutex_unlock(&h->tablesLock);
    return most;
}

int spgpuSpmvHold(spgpuHandle_t pHandle, const int* rP)
{
    if (!pHandle || !rP)
        return SPGPU_UNSPECIFIED;
    SpgpuPrivateHandle* h = spgpuPrivate(pHandle);
    if (!h->plans || !spgpuTuning()->plan)
        return SPGPU_UNSUPPORTED;
    /* inside a capture the call neither waits nor touches the stream: the capture goes on undisturbed */
    if (spgpuStreamCapturing(h->pub.currentStream)) {
        (void)hipGetLastError();
        return SPGPU_UNSUPPORTED;
    }
    if (heldRecords(h, rP, 1) < 0)
        return SPGPU_UNSUPPORTED;
    (void)hipStreamSynchronize(h->pub.currentStream); /* like Prepare / Freeze / Adopt: what was queued to build the records has landed */
    return SPGPU_SUCCESS;
}

int spgpuSpmvRelease(spgpuHandle_t pHandle, const int* rP)
{
    if (!pHandle || !rP)
        return SPGPU_UNSPECIFIED;
    SpgpuPrivateHandle* h = spgpuPrivate(pHandle);
    if (!h->plans)
        return SPGPU_UNSUPPORTED;
    return heldRecords(h, rP, -1) > 0 ? SPGPU_SUCCESS : SPGPU_UNSUPPORTED;
}

int spgpuSpmvHolds(spgpuHandle_t pHandle, const int* rP)
{
    if (!pHandle || !rP)
        return 0;
    SpgpuPrivateHandle* h = spgpuPrivate(pHandle);
    return h->plans ? heldRecords(h, rP, 0) : 0;
}

/* spgpu?SpmvFreeze's counterpart (include/spgpu/tuning.h): the plans of the matrix with this index array lose their 16-bit copies
 * -- retired whole, the next SpMV analyses the matrix again. */
int spgpuSpmvThaw(spgpuHandle_t pHandle, const int* rP)
{
    SpgpuPrivateHandle* h = spgpuPrivate(pHandle);
    int thawed = 0;
    if (!h || !h->plans || !rP)
        return SPGPU_UNSPECIFIED;
    if (heldRecords(h, rP, 0) > 0)
        return SPGPU_IN_USE; /* a captured graph may still replay on the records: nothing is freed */
    {
        /* an adopted matrix: the plan of its ordered copy goes first (keyed by the copy's arrays), then the copy -- behind a
         * device-wide wait: SpMVs in flight read it */
        SpgpuAdopted gone[SPGPU_ADOPTED];
        const int n = spgpuAdoptedRemove(pHandle, rP, gone);
        if (n > 0)
            hipDeviceSynchronize();
        for (int i = 0; i < n; ++i) {
            (void)spgpuSpmvThaw(pHandle, gone[i].indices);
            freeAdopted(&gone[i]);
            thawed += 1;
        }
    }
    pthread_mutex_lock(&h->tablesLock);
    for (int i = 0; i < SPGPU_PLANS; ++i) {
        SpgpuSpmvPlan* p = &h->plans[i];
        if (p->rows > 0 && p->rP == (const void*)rP && p->packed) {
            spgpuPlanRetire(pHandle, p);
            thawed += 1;
        }
    }
    spgpuPlanCountFrozenSlabs(pHandle);
    pthread_mutex_unlock(&h->tablesLock);
    return thawed ? SPGPU_SUCCESS : SPGPU_UNSUPPORTED;
}

long long spgpuSpmvFrozenBytes(spgpuHandle_t pHandle)
{
    SpgpuPrivateHandle* h = spgpuPrivate(pHandle);
    long long bytes = 0;
    if (!h || !h->plans)
        return 0;
    pthread_mutex_lock(&h->tablesLock);
    for (int i = 0; h->adopted && i < SPGPU_ADOPTED; ++i)
        bytes += h->adopted[i].rows > 0 ? h->adopted[i].bytes : 0;
    for (int i = 0; i < SPGPU_PLANS; ++i)
        bytes += h->plans[i].packed ? h->plans[i].packedBytes : 0;
    pthread_mutex_unlock(&h->tablesLock);
    return bytes;
}
