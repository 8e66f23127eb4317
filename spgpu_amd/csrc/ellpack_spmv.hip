/*
 * ELL and HELL SpMV for gfx950 (MI355X):  z = alpha*A*x + beta*y.
 *
 * C ABI: spgpu{S,D,C,Z}hellspmv (include/spgpu/hell.h, reference hell.h:45-169)
 *        spgpu{S,D,C,Z}ellspmv  (include/spgpu/ell.h,  reference ell.h:46-173)
 * Behaviour follows the reference dispatchers/kernels
 * (kernels/hell_spmv_base.cuh:103-157, hell_spmv_base_template.cuh:19-357,
 *  kernels/ell_spmv_base.cuh:99-146, ell_spmv_base_template.cuh:102-425,
 *  ell_spmv_base_nors.cuh:17-340); the kernel design (slab_spmv.hip.h) is new.
 * This file is the dispatch and the C ABI; the kernels live in the *.hip.h it includes (slab_spmv.hip.h carries the wavefront design).
 */
#include "numeric.hip.h"
#include <type_traits>
#include "spgpu_internal.h"
#include "slab_args.hip.h"

#include "spgpu/ell.h"
#include "spgpu/hell.h"

#include <stdio.h>
#include <stdlib.h>

namespace spgpu {

#include "slab_spmv.hip.h"
#include "deep_items.hip.h"
#include "form_probe.hip.h"
#include "sweep_spmv.hip.h"

#ifdef SPGPU_TRACE_BLOCKS
__device__ unsigned long long* spgpuTraceBuffer;
#endif
#include "ragged_spmv.hip.h"

/* ---- host side ----------------------------------------------------------- */

static bool alignedTo(const void* p, size_t bytes)
{
    return ((uintptr_t)p % bytes) == 0;
}

/* One launch of slabSpmvKernel: the kernel's own template parameter list, a wavefront per group of (64 / PH) * RPL rows. */
template <typename T, int RPL, int PH, bool IS_HELL, bool NT, int UNROLL, bool PIPE, bool TAIL, bool STRIPS = false,
          int BLOCK = kBlockThreads, int TILE_BYTES = 0, int TAIL_EVERY = 0, bool PACKED = false>
static void launchSlabKernel(hipStream_t stream, const SlabArgs<T>& a)
{
    constexpr int GROUP_ROWS = (kWave / PH) * RPL;
    constexpr int WAVES = BLOCK / kWave;
    const long long groups = ((long long)a.rows + GROUP_ROWS - 1) / GROUP_ROWS;
    const unsigned blocks = (unsigned)((groups + WAVES - 1) / WAVES);
    hipLaunchKernelGGL((slabSpmvKernel<T, RPL, PH, IS_HELL, NT, UNROLL, PIPE, TAIL, STRIPS, BLOCK, TILE_BYTES, TAIL_EVERY, PACKED>),
                       dim3(blocks), dim3(BLOCK), 0, stream, a);
}

/* The x-tile forms.  Workgroup size and tile size go together: the tile has to hold the columns of the workgroup's
 * rows, and LDS (160 KiB per CU) divided by the tile is the number of workgroups a CU overlaps.  The coefficient/index
 * streams always carry the non-temporal hint here.
 * Same summation order as the type's gather / strip kernel (launchSlabFamily), so that the form AUTO settles on never
 * changes a bit of the result: 8-byte elements walk whole rows and consider the tail every 8 columns; fp32 keeps its
 * 8 phases x 2 columns; complex fp64 and the narrow form of every type their 2 phases.  The 8-byte types walk whole rows (PH 1) with 4
 * slab columns per stage -- half the stage of the gather kernel: LDS gathers are short, and at 8 the kernel needs 148 VGPRs, which
 * leaves room for one 512-lane workgroup per CU only.  32 KiB of x per workgroup. */
template <typename T, int RPL, bool IS_HELL>
static void launchTiled(hipStream_t stream, const SlabArgs<T>& a)
{
    /* RPL == 1 (a layout the wide kernels cannot read): the two phases x 4 columns of the narrow gather kernel, without tail rows, for every
     * type -- XTILE on such a matrix gives the bits of GATHER on it (include/spgpu/tuning.h: the form never changes a bit) */
    constexpr int PH = (sizeof(T) == 16 || RPL == 1) ? 2 : 1;
    if constexpr (sizeof(T) == 4 && RPL == 4)
        launchSlabKernel<T, RPL, 2 * RPL, IS_HELL, true, 2, true, true, false, 512, 32768>(stream, a);
    else if constexpr (sizeof(T) == 8 && RPL == 2)
        launchSlabKernel<T, RPL, 1, IS_HELL, true, 4, true, true, false, 256, 32768, 8>(stream, a);
    else
        launchSlabKernel<T, RPL, PH, IS_HELL, true, 4, true, PH == 1, false, 256, 32768>(stream, a);
}

constexpr int kAutoSweepRows = 2 * 1024 * 1024; /* AUTO: the SWEEP form wants a grid that fills the chip (8 192 rows per workgroup); measured, scattered
                                                  * fp64, 16 and 32 per row: 1 Mi rows 1.5 x SLOWER than the gathers (x fits the L2s), 2 Mi ... 16 Mi rows 0.61 ... 0.89 x their
                                                  * time (profiles/r04_exp_sweep_rows.txt) */

/* SWEEP: 32 rows per lane (16 for 16-byte elements), at most 2 048 workgroups.  8-byte elements add in the order of their
 * default kernel (whole-wave tail rows), the others in one phase. */
template <typename T, int VEC, bool IS_HELL>
static void launchSweep(hipStream_t stream, const SlabArgs<T>& a)
{
    constexpr int PACKS = sizeof(T) == 16 ? 16 : 32 / VEC;
    constexpr bool TAIL = sizeof(T) == 8;
    const long long packs = ((long long)a.rows + VEC - 1) / VEC;
    long long blocks = (packs + (long long)kBlockThreads * PACKS - 1) / ((long long)kBlockThreads * PACKS);
    blocks = blocks > 2048 ? 2048 : blocks;
    if (isNotZero(a.beta))
        hipLaunchKernelGGL((sweepSpmvKernel<T, VEC, PACKS, IS_HELL, true, TAIL>), dim3((unsigned)blocks), dim3(kBlockThreads), 0, stream, a);
    else
        hipLaunchKernelGGL((sweepSpmvKernel<T, VEC, PACKS, IS_HELL, false, TAIL>), dim3((unsigned)blocks), dim3(kBlockThreads), 0, stream, a);
}

/* Right behind a DEEP kernel.  Fixed grids (the number of items is known on the device only): with nothing
 * registered both kernels read the header and leave. */
template <typename T, int RPL, bool IS_HELL>
static void launchDeep(hipStream_t stream, const SlabArgs<T>& a)
{
    constexpr int PH = kWave / (32 / RPL);
    constexpr int UNROLL = 32 / PH; /* 32 columns per stage, two stages per item */
    hipLaunchKernelGGL((deepItemsKernel<T, RPL, IS_HELL, UNROLL, kDeepChunk>), dim3(SPGPU_DEEP_ITEMS / (kBlockThreads / kWave)), dim3(kBlockThreads), 0, stream, a);
    hipLaunchKernelGGL((deepFinishKernel<T>), dim3(256), dim3(kBlockThreads), 0, stream, a);
}

/* Short rows (see launchRowsAsTheyCome): a lane walks whole rows, 4 columns per stage, no prefetch; 8-byte element types. */
template <typename T, int RPL, bool IS_HELL>
static void launchLean(hipStream_t stream, const SlabArgs<T>& a)
{
    launchSlabKernel<T, RPL, 1, IS_HELL, true, 4, false, true, false, kBlockThreads, 0, 8>(stream, a);
}

/* The probe of the type's default kernel shape (launchSlabFamily): D/C walk whole rows, 8 columns per stage; S 8 phases x 2. */
template <typename T, bool IS_HELL>
static void launchFormProbe(hipStream_t stream, const SlabArgs<T>& a, bool wideOk)
{
    constexpr int WIDE = 16 / (int)sizeof(T);
    if constexpr (WIDE > 1) {
        if (wideOk) {
            if constexpr (sizeof(T) == 4)
                hipLaunchKernelGGL((formProbeKernel<T, WIDE, 2 * WIDE, IS_HELL, 2 * WIDE * 2>), dim3(3), dim3(kWave), 0, stream, a);
            else
                hipLaunchKernelGGL((formProbeKernel<T, WIDE, 1, IS_HELL, 8>), dim3(3), dim3(kWave), 0, stream, a);
            return;
        }
    }
    hipLaunchKernelGGL((formProbeKernel<T, 1, 2, IS_HELL, 8>), dim3(3), dim3(kWave), 0, stream, a);
}

#include "frozen_slab.hip.h"

/* Rows of a wavefront of the type's wide kernel (launchRowsAsTheyCome): fp32 runs 8 phases, the 8-byte types one. */
template <typename T> constexpr int kWide = 16 / (int)sizeof(T);
template <typename T> constexpr int kWideGroupRows = sizeof(T) == 4 ? (kWave / (2 * kWide<T>)) * kWide<T> : kWave * kWide<T>;

/* A lane reads WIDE = 16 / sizeof(T) consecutive rows of a slab column with one 16-byte load: the strip must not straddle a
 * hack (HELL) or run past the pitch (ELL), and the streams must be 16-byte aligned. */
template <typename T, bool IS_HELL>
static bool wideLayout(const SlabArgs<T>& a)
{
    constexpr int WIDE = 16 / (int)sizeof(T);
    const long long stripRows = ((long long)a.rows + WIDE - 1) / WIDE * WIDE;
    const bool layoutOk = IS_HELL ? (a.hackSize > 0 && a.hackSize % WIDE == 0)
                                  : (a.valStride >= stripRows && a.idxStride >= stripRows);
    return layoutOk && alignedTo(a.cM, 16) && alignedTo(a.rP, 4 * WIDE) && a.valStride % WIDE == 0 && a.idxStride % WIDE == 0;
}

/* Deep split (ragged_spmv.hip.h, the deep list): on when the caller passes a row order -- rows ordered by length are what
 * one does to a ragged matrix, and then whole hacks are deep -- or when SPGPU_DEEP_SPLIT says so.  Sets the deep fields of `a`:
 * the list's pointers where the current stream has one, else they stay NULL as matrixArgs left them.  true: the call takes the
 * ordered path (launchOrdered); *noDeepList: it does so without a list, because this stream of the handle has none. */
template <typename T>
static bool attachDeepList(spgpuHandle_t handle, SlabArgs<T>& a, bool wideOk, SpgpuDeepList* list, bool* noDeepList)
{
    const SpgpuTuning* tune = spgpuTuning();
    const bool deepSplit = (tune->deepSplit >= 0 ? tune->deepSplit != 0 : a.rIdx != nullptr) && wideOk;
    a.deepCap = tune->deepCap > 0 ? tune->deepCap : 256;
    a.deepKeep = tune->deepKeep >= 0 && tune->deepKeep < a.deepCap ? tune->deepKeep : a.deepCap;
    a.deepChunk = kDeepChunk;
    a.deepOverflow = spgpuDeepOverflowWords(handle);
    *noDeepList = false;
    list->idle = nullptr;
    if (!deepSplit)
        return false;
    if (spgpuDeepScratch(handle, list) == SPGPU_SUCCESS) {
        a.deepHeader = list->header;
        a.deepEntries = list->entries;
        a.deepItems = list->items;
        a.deepPartials = static_cast<T*>(list->partials);
        a.deepItemSums = static_cast<T*>(list->itemSums);
    } else {
        *noDeepList = true;
    }
    return true;
}

/* Which of the queue kernel's two product shapes (launchRagged)?  orderedProbeKernel answers; the answer is kept with AUTO's
 * per-matrix words and read without synchronisation: a first call runs the 1 024-row shape, which is never far off.
 * wait (Prepare, Freeze): a first call waits for the answer a second call would have found. */
template <typename T, bool IS_HELL>
static int orderedShape(spgpuHandle_t handle, hipStream_t stream, const SlabArgs<T>& a, bool wait)
{
    int calls = 0, tag = 0;
    int* seen = spgpuFormFeedback(handle, a.rP, a.rows, &calls, &tag);
    int said = spgpuFeedbackSaid(((volatile int*)seen)[3], tag);
    if (said == 0 || calls % 64 == 0)
        hipLaunchKernelGGL((orderedProbeKernel<IS_HELL>), dim3(1), dim3(kWave), 0, stream, a.rP, a.rS, a.hackOffsets, a.rIdx, a.hackSize,
                           a.idxStride, a.maxNnz, a.rows, a.baseIndex, seen + 3, tag);
    if (wait && said == 0 && hipStreamSynchronize(stream) == hipSuccess)
        said = spgpuFeedbackSaid(((volatile int*)seen)[3], tag);
    return said == 4 || said == 6 ? 4 : 0; /* 6: the blocks are the windows of an aligned order */
}

/* The ordered path: the queue-driven kernel for rows ordered by length (ragged_spmv.hip.h); x through an LDS tile unless the
 * caller asked for plain gathers.  A matrix seen before has a plan (planned_spmv.hip): one launch, the deep sub-groups in
 * workgroups of their own, no list.  Otherwise the queue kernel registers them in the stream's deep list and the deep kernels
 * follow.  noDeepList: this stream of the handle has no deep list (every list belongs to a stream with work in flight, or the
 * allocation failed): the same kernel family without any state -- the matrix' plan if it is ready, else no plan at all (every
 * deep sub-group worked off by its own block).  Same bits in every case.
 * Returns, for Prepare / Freeze: the next SpMV on these arrays runs from a plan / the matrix is frozen. */
template <typename T, bool IS_HELL>
static bool launchOrdered(spgpuHandle_t handle, hipStream_t stream, SlabArgs<T>& a, int form, const SpgpuDeepList& list, bool noDeepList, SpmvCall call)
{
    constexpr int WIDE = 16 / (int)sizeof(T);
    const bool tiledForm = form != SPGPU_SPMV_FORM_GATHER;
    spgpuNoteSpmvForm(handle, tiledForm ? SPGPU_SPMV_FORM_XTILE : SPGPU_SPMV_FORM_GATHER);
    int shape = spgpuTuning()->raggedShape;
    if (shape == 0 && tiledForm && a.rIdx != nullptr && sizeof(T) <= 8)
        shape = orderedShape<T, IS_HELL>(handle, stream, a, call != SpmvCall::Run);
    if (noDeepList && shape != 4)
        shape = 0;
    const bool plannable = !tiledForm || shape == 0 || shape == 4;
    if (call != SpmvCall::Run)
        return plannable && launchPlanned<T, IS_HELL>(handle, stream, a, shape, tiledForm, false, call);
    if (plannable && launchPlanned<T, IS_HELL>(handle, stream, a, shape, tiledForm, noDeepList, SpmvCall::Run))
        return true;
    /* ELL says how long its longest row is: when none can exceed the cap nothing registers and the two launches behind
     * the main kernel (~5 us each when empty) are left out; HELL does not say */
    const bool deepPossible = IS_HELL || a.maxNnz > a.deepCap;
    const bool deepKernels = launchRagged<T, WIDE, IS_HELL, true>(stream, a, shape, tiledForm);
    if (deepPossible && deepKernels)
        launchDeep<T, WIDE, IS_HELL>(stream, a);
    if (list.idle) {
        /* complete = the list has no user (core.c: a list may change hands) -- unless this launch is being captured: a graph
         * carries the list's addresses and may be replayed at any time, so the list stays with this stream for good */
        if (!spgpuStreamCapturing(stream))
            (void)hipEventRecord(list.idle, stream);
        else
            spgpuDeepListPin(handle);
    }
    return true;
}

/* What AUTO (or the caller's hint) decided for rows as they come: the strip-capable kernel; AUTO's x tile; AUTO's SWEEP form;
 * formProbeKernel in front of this launch (its answer is for later calls). */
struct FormVote {
    bool strips, autoTile, autoSweep, probeBehind;
};

/* Strip x loads (consume<STRIPS>): which form a matrix runs in is learnt from the kernel itself.  The
 * strip-capable kernel's sample wavefronts write "ran as strips / as gathers" into pinned host memory; a
 * later call on the same matrix (same rP, same rows) reads that -- no synchronisation, whatever is there --
 * and takes the gather-only kernel when at least two of the three samples said gathers.  Both kernels are
 * correct for every matrix; a stale or missing answer only costs speed.  SPGPU_X_STRIPS = 0 / 1 fixes the form.
 * eligible: wide layout, more than one row per lane, no x tile asked for.  Leaves the report words in a.feedback / a.feedbackTag. */
template <typename T>
static FormVote voteForm(spgpuHandle_t handle, SlabArgs<T>& a, int form, bool eligible)
{
    FormVote vote{false, false, false, false};
    a.feedback = nullptr;
    a.tileSpanLimit = (long long)(32768 / sizeof(T)) * 5 / 4; /* 1.25 x the tile (launchTiled) */
    if (!eligible)
        return vote;
    if (form != SPGPU_SPMV_FORM_AUTO) {
        vote.strips = form == SPGPU_SPMV_FORM_STRIPS;
        return vote;
    }
    int calls = 0, tag = 0;
    int* seen = spgpuFormFeedback(handle, a.rP, a.rows, &calls, &tag);
    a.feedbackTag = tag;
    int gathers = 0, local = 0, sweeps = 0;
    for (int q = 0; q < 3; ++q) {
        const int said = spgpuFeedbackSaid(((volatile int*)seen)[q], tag);
        gathers += said == 1 ? 1 : 0;
        local += said == 3 ? 1 : 0;
        sweeps += said == 4 ? 1 : 0;
    }
    /* two of three samples decide: scattered -> gathers; inside a window -> the LDS tile; otherwise (strips, or
     * nothing known yet) the strip-capable kernel */
    vote.autoTile = local >= 2;
    vote.strips = gathers + local + sweeps < 2;
    /* scattered over all of x, ascending inside the rows, rows about equally long (only the probe says so: answer 4):
     * the SWEEP form -- same bits as the default kernel of the 8-byte types; it needs rows for a resident grid */
    vote.autoSweep = sweeps >= 2 && !vote.autoTile && sizeof(T) == 8 && spgpuTuning()->autoSweep != 0 && !a.rIdx && a.rows >= kAutoSweepRows;
    a.feedback = seen; /* the strip-capable kernel's sample wavefronts report (it is what a new matrix runs first) */
    /* the other forms do not (see slabSpmvKernel): with every fourth call of theirs three wavefronts look at the
     * matrix again -- another one may live at this address by now -- and with the first of them (the samples know
     * strips, a window and "neither"; whether "neither" is a matrix for the SWEEP form only the probe finds out) */
    vote.probeBehind = !vote.strips && (calls % 4 == 0 || calls == 1);
    return vote;
}

/* The launches for rows as they come.  Kernel shape, measured on MI355X, 10 M rows x 32 nnz (profiles/): wide where the layout
 * allows it (wideOk), with the next stage prefetched AFTER the current gathers are issued and whole-wave tail rows -- D/C fastest
 * with a lane walking whole rows, 8 slab columns per stage (banded 5.9 TB/s, windowed columns +13 % over prefetch-before); S
 * (PHASED) with 8 phases x 2 columns (5.4-6.0 TB/s).  16-byte elements (Z) and unaligned streams run narrow: RPL = 1 with 2
 * phases x 4 columns (5.9 TB/s).  The coefficient/index streams carry the non-temporal hint. */
template <typename T, bool IS_HELL>
static void launchRowsAsTheyCome(spgpuHandle_t handle, hipStream_t stream, SlabArgs<T>& a, int form, bool wideOk, bool tiled, const FormVote& vote)
{
    constexpr int WIDE = 16 / (int)sizeof(T);
    constexpr bool PHASED = sizeof(T) == 4;
    spgpuNoteSpmvForm(handle, (tiled || vote.autoTile) ? SPGPU_SPMV_FORM_XTILE
                                                       : (vote.autoSweep ? SPGPU_SPMV_FORM_SWEEP : (vote.strips ? SPGPU_SPMV_FORM_STRIPS : SPGPU_SPMV_FORM_GATHER)));
    if (vote.probeBehind)
        launchFormProbe<T, IS_HELL>(stream, a, wideOk); /* 3 wavefronts; its answer is for later calls */
    if (vote.autoSweep) {
        if constexpr (WIDE > 1) {
            a.wideIO = alignedTo(a.z, 16) && alignedTo(a.y, 16);
            a.feedback = nullptr;
            launchSweep<T, WIDE, IS_HELL>(stream, a);
            return;
        }
    }
    if (!vote.strips)
        a.feedback = nullptr;
    if (wideOk) {
        a.wideIO = alignedTo(a.z, 16) && alignedTo(a.y, 16);
        if constexpr (WIDE > 1) {
            if (tiled || vote.autoTile) {
                launchTiled<T, WIDE, IS_HELL>(stream, a);
            } else if (!PHASED && a.avgNnzPerRow > 0 && a.avgNnzPerRow <= 8 && form == SPGPU_SPMV_FORM_AUTO && (IS_HELL || a.maxNnz <= 16)) {
                /* the caller says the rows are short (avgNnzPerRow: the reference's own tuning hint, which picks its
                 * threads-per-row shape, hell_spmv_base_template.cuh:306-325): such a row is one stage, and a kernel
                 * without the prefetch ring needs a third of the registers -- all wavefronts of a 1 M-row system are
                 * resident at once instead of queueing in three rounds (19.4 -> 17.4 us on configs[0]).  Same order of
                 * additions (the tail switch is considered every 8 columns, as in the default kernel:
                 * tests/test_gpu_spmv.py::test_short_row_hint_same_bits pins that on rows of 0 .. 300 entries).  ELL says how long
                 * its longest row is: beyond two stages the prefetching kernel stays, whatever the average; HELL has only the hint. */
                spgpuNoteSpmvForm(handle, SPGPU_SPMV_FORM_GATHER);
                a.feedback = nullptr;
                launchLean<T, WIDE, IS_HELL>(stream, a);
            } else {
                /* the gather and strip forms: the next stage prefetched behind the current gathers; a frozen matrix reads its 16-bit indices */
                findFrozenSlab(handle, stream, a, kWideGroupRows<T>);
                constexpr int PH = PHASED ? 2 * WIDE : 1, UNROLL = PHASED ? 2 : 8;
                if (a.planPacked && vote.strips)
                    launchSlabKernel<T, WIDE, PH, IS_HELL, true, UNROLL, true, true, true, kBlockThreads, 0, 0, true>(stream, a);
                else if (a.planPacked)
                    launchSlabKernel<T, WIDE, PH, IS_HELL, true, UNROLL, true, true, false, kBlockThreads, 0, 0, true>(stream, a);
                else if (vote.strips)
                    launchSlabKernel<T, WIDE, PH, IS_HELL, true, UNROLL, true, true, true>(stream, a);
                else
                    launchSlabKernel<T, WIDE, PH, IS_HELL, true, UNROLL, true, true>(stream, a);
            }
            return;
        }
    }
    a.wideIO = 1; /* RPL == 1: element access is always aligned */
    if (tiled)
        launchTiled<T, 1, IS_HELL>(stream, a);
    else
        launchSlabKernel<T, 1, 2, IS_HELL, true, 4, true, false>(stream, a);
}

/* The dispatch of every ELL / HELL SpMV, and of Prepare and Freeze (SpmvCall).  Run: launches the SpMV.  Prepare / Freeze:
 * true = the next SpMV on these arrays runs from a plan / the matrix is frozen; false = this kind of call has none. */
template <typename T, bool IS_HELL>
static bool launchSlabFamily(spgpuHandle_t handle, const SlabArgs<T>& in, SpmvCall call = SpmvCall::Run)
{
    if (in.rows <= 0)
        return false;
    SlabArgs<T> a = in;
    hipStream_t stream = handle->currentStream;
    constexpr int WIDE = 16 / (int)sizeof(T);
    const bool wideOk = wideLayout<T, IS_HELL>(a);
    a.tailLanes = kTailLanes;
    /* How x is fetched (include/spgpu/tuning.h): the handle's hint, overridden by SPGPU_X_STRIPS. */
    int form = spgpuGetSpmvForm(handle);
    if (spgpuTuning()->xStrips >= 0)
        form = spgpuTuning()->xStrips ? SPGPU_SPMV_FORM_STRIPS : SPGPU_SPMV_FORM_GATHER;
    if (form == SPGPU_SPMV_FORM_SWEEP) {
        /* the caller's choice for scattered columns that ascend inside a row; needs 16-byte slab accesses and no row order */
        if (wideOk && !a.rIdx) {
            if (call != SpmvCall::Run)
                return false;
            a.wideIO = alignedTo(a.z, 16) && alignedTo(a.y, 16);
            a.feedback = nullptr;
            spgpuNoteSpmvForm(handle, SPGPU_SPMV_FORM_SWEEP);
            launchSweep<T, WIDE, IS_HELL>(stream, a);
            return true;
        }
        form = SPGPU_SPMV_FORM_AUTO;
    }
    const bool tiled = form == SPGPU_SPMV_FORM_XTILE;
    SpgpuDeepList list;
    bool noDeepList;
    if (attachDeepList(handle, a, wideOk, &list, &noDeepList))
        return launchOrdered<T, IS_HELL>(handle, stream, a, form, list, noDeepList, call);
    if (call != SpmvCall::Run) {
        /* (the forms below learn what they need from their own launches) -- Freeze of a matrix without a row order: the default
         * kernels' 16-bit index copy, counted per group of rows of a wavefront of the wide kernel */
        if constexpr (WIDE > 1) {
            if (call == SpmvCall::Freeze && !a.rIdx && wideOk && !tiled)
                return freezeSlab<IS_HELL>(handle, stream, planKey(a, nullptr, 0, -kWideGroupRows<T>));
        }
        return false;
    }
    const FormVote vote = voteForm(handle, a, form, wideOk && WIDE > 1 && !tiled);
    launchRowsAsTheyCome<T, IS_HELL>(handle, stream, a, form, wideOk, tiled, vote);
    return true;
}

/* The matrix part of the kernels' arguments; everything else is zero / NULL, and the dispatch sets only what the path it takes reads. */
template <typename T>
static SlabArgs<T> matrixArgs(const void* cM, const int* rP, int hackSize, const int* hackOffsets, long long valStride, long long idxStride,
                              const int* rS, const int* rIdx, int maxNnz, int rows, int baseIndex)
{
    SlabArgs<T> a{};
    a.cM = static_cast<const T*>(cM);
    a.rP = rP;
    a.rS = rS;
    a.rIdx = rIdx;
    a.hackOffsets = hackOffsets;
    a.rows = rows;
    a.baseIndex = baseIndex;
    a.hackSize = hackSize;
    a.maxNnz = maxNnz;
    a.valStride = valStride;
    a.idxStride = idxStride;
    return a;
}

template <typename T, bool IS_HELL, typename ApiT>
static void runSpmv(spgpuHandle_t handle, SlabArgs<T>& a, ApiT* z, const ApiT* y, ApiT alpha, const ApiT* x, ApiT beta, int avgNnzPerRow)
{
    static_assert(sizeof(T) == sizeof(ApiT), "ABI type and device type must have one layout");
    a.z = reinterpret_cast<T*>(z);
    a.y = reinterpret_cast<const T*>(y);
    a.x = reinterpret_cast<const T*>(x);
    __builtin_memcpy(&a.alpha, &alpha, sizeof(T));
    __builtin_memcpy(&a.beta, &beta, sizeof(T));
    a.avgNnzPerRow = avgNnzPerRow;
    (void)launchSlabFamily<T, IS_HELL>(handle, a);
}

template <typename T, typename ApiT>
static void hellSpmv(spgpuHandle_t handle, ApiT* z, const ApiT* y, ApiT alpha, const ApiT* cM, const int* rP,
                     int hackSize, const int* hackOffsets, const int* rS, const int* rIdx, int rows,
                     const ApiT* x, ApiT beta, int baseIndex, int avgNnzPerRow = 0)
{
    /* an ADOPTED matrix (spgpuHellSpmvAdopt, adopted_hell.hip): the call runs on the library's ordered copy and writes z through the
     * copy's row order -- z in the caller's row order, as ever */
    if (!rIdx) {
        const SpgpuAdopted* copy = spgpuAdoptedFind(handle, handle->currentStream, cM, rP, rS, hackOffsets, rows, hackSize, baseIndex, 0, 0);
        if (copy && spgpuSizeOf((spgpuType_t)copy->type) == sizeof(T)) { /* (adopted as another type: the call runs on the caller's arrays) */
            cM = static_cast<const ApiT*>(copy->values);
            rP = copy->indices;
            hackOffsets = copy->hackOffsetsOrdered;
            rS = copy->lengths;
            rIdx = copy->order;
        }
    }
    SlabArgs<T> a = matrixArgs<T>(cM, rP, hackSize, hackOffsets, hackSize, hackSize, rS, rIdx, 0, rows, baseIndex);
    runSpmv<T, true>(handle, a, z, y, alpha, x, beta, avgNnzPerRow);
    spgpuDebugCheck(handle, "hellspmv");
}

template <typename T, typename ApiT>
static void ellSpmv(spgpuHandle_t handle, ApiT* z, const ApiT* y, ApiT alpha, const ApiT* cM, const int* rP,
                    int cMPitch, int rPPitch, const int* rS, const int* rIdx, int maxNnzPerRow, int rows,
                    const ApiT* x, ApiT beta, int baseIndex, int avgNnzPerRow = 0)
{
    /* an ADOPTED ELL matrix (spgpuEllSpmvAdopt, adopted_hell.hip): the call runs on the library's ordered HELL copy */
    if (!rIdx && rS) {
        const SpgpuAdopted* copy = spgpuAdoptedFind(handle, handle->currentStream, cM, rP, rS, nullptr, rows, 0, baseIndex, cMPitch, rPPitch);
        if (copy && spgpuSizeOf((spgpuType_t)copy->type) == sizeof(T)) {
            hellSpmv<T, ApiT>(handle, z, y, alpha, static_cast<const ApiT*>(copy->values), copy->indices, 32, copy->hackOffsetsOrdered, copy->lengths,
                              copy->order, rows, x, beta, baseIndex, avgNnzPerRow);
            return;
        }
    }
    SlabArgs<T> a = matrixArgs<T>(cM, rP, 0, nullptr, cMPitch, rPPitch, rS, rIdx, maxNnzPerRow, rows, baseIndex);
    runSpmv<T, false>(handle, a, z, y, alpha, x, beta, avgNnzPerRow);
    spgpuDebugCheck(handle, "ellspmv");
}

/* spgpu?SpmvPrepare / spgpu?SpmvFreeze (include/spgpu/tuning.h): the dispatch of an SpMV on these arrays, with nothing multiplied */
template <typename T, bool IS_HELL>
static int prepareSpmv(spgpuHandle_t handle, const void* cM, const int* rP, int hackSize, const int* hackOffsets, long long valStride, long long idxStride,
                       const int* rS, const int* rIdx, int maxNnz, int rows, int baseIndex, bool freeze)
{
    const SlabArgs<T> a = matrixArgs<T>(cM, rP, hackSize, hackOffsets, valStride, idxStride, rS, rIdx, maxNnz, rows, baseIndex);
    return launchSlabFamily<T, IS_HELL>(handle, a, freeze ? SpmvCall::Freeze : SpmvCall::Prepare) ? SPGPU_SUCCESS : SPGPU_UNSUPPORTED;
}

template <bool IS_HELL>
static int prepareSpmvOfType(spgpuHandle_t handle, spgpuType_t type, const void* cM, const int* rP, int hackSize, const int* hackOffsets, long long valStride,
                             long long idxStride, const int* rS, const int* rIdx, int maxNnz, int rows, int baseIndex, bool freeze = false)
{
    if (!handle || !rP || !cM || rows < 0)
        return SPGPU_UNSPECIFIED;
    switch (type) {
    case SPGPU_TYPE_FLOAT: return prepareSpmv<float, IS_HELL>(handle, cM, rP, hackSize, hackOffsets, valStride, idxStride, rS, rIdx, maxNnz, rows, baseIndex, freeze);
    case SPGPU_TYPE_DOUBLE: return prepareSpmv<double, IS_HELL>(handle, cM, rP, hackSize, hackOffsets, valStride, idxStride, rS, rIdx, maxNnz, rows, baseIndex, freeze);
    case SPGPU_TYPE_COMPLEX_FLOAT: return prepareSpmv<cfloat, IS_HELL>(handle, cM, rP, hackSize, hackOffsets, valStride, idxStride, rS, rIdx, maxNnz, rows, baseIndex, freeze);
    case SPGPU_TYPE_COMPLEX_DOUBLE: return prepareSpmv<cdouble, IS_HELL>(handle, cM, rP, hackSize, hackOffsets, valStride, idxStride, rS, rIdx, maxNnz, rows, baseIndex, freeze);
    default: return SPGPU_UNSPECIFIED;
    }
}

#include "ell_csput.hip.h"

template <typename T, typename ApiT>
static void ellCsput(spgpuHandle_t handle, ApiT* cM, const int* rP, int cMPitch, int rPPitch, const int* rS, int nnz,
                     const int* aI, const int* aJ, const ApiT* aVal, int baseIndex)
{
    if (nnz <= 0)
        return;
    const unsigned blocks = (unsigned)(((long long)nnz + kBlockThreads - 1) / kBlockThreads);
    hipLaunchKernelGGL((ellCsputKernel<T>), dim3(blocks), dim3(kBlockThreads), 0, handle->currentStream,
                       reinterpret_cast<T*>(cM), rP, (long long)cMPitch, (long long)rPPitch, rS, nnz, aI, aJ,
                       reinterpret_cast<const T*>(aVal), baseIndex);
    spgpuDebugCheck(handle, "ellcsput");
}

/* ---- spgpuHellSpmvForm / spgpuEllSpmvForm (include/spgpu/tuning.h): the probe, synchronously ---- */
template <typename T, bool IS_HELL>
static int analyseForm(spgpuHandle_t handle, const int* rP, int hackSize, const int* hackOffsets, long long idxStride, const int* rS,
                       int maxNnz, int rows, int baseIndex)
{
    if (rows <= 0)
        return SPGPU_SPMV_FORM_GATHER;
    constexpr int WIDE = 16 / (int)sizeof(T);
    SlabArgs<T> a = matrixArgs<T>(nullptr, rP, hackSize, hackOffsets, idxStride, idxStride, rS, nullptr, maxNnz, rows, baseIndex);
    a.tileSpanLimit = (long long)(32768 / sizeof(T)) * 5 / 4;
    int* seen = spgpuAnalyseWords(handle);
    seen[0] = seen[1] = seen[2] = 0;
    a.feedback = seen;
    a.feedbackTag = 0;
    const bool wide = IS_HELL ? (hackSize > 0 && hackSize % WIDE == 0) : true;
    launchFormProbe<T, IS_HELL>(handle->currentStream, a, wide);
    if (hipStreamSynchronize(handle->currentStream) != hipSuccess)
        return SPGPU_SPMV_FORM_AUTO;
    int strips = 0, local = 0, sweeps = 0;
    for (int q = 0; q < 3; ++q) {
        strips += seen[q] == 2;
        local += seen[q] == 3;
        sweeps += seen[q] == 4;
    }
    if (sweeps >= 2 && sizeof(T) == 8 && rows >= kAutoSweepRows) /* where AUTO itself would take it */
        return SPGPU_SPMV_FORM_SWEEP;
    return strips >= 2 ? SPGPU_SPMV_FORM_STRIPS : (local >= 2 ? SPGPU_SPMV_FORM_XTILE : SPGPU_SPMV_FORM_GATHER);
}

template <bool IS_HELL>
static int analyseFormOfType(spgpuHandle_t handle, spgpuType_t type, const int* rP, int hackSize, const int* hackOffsets, long long idxStride,
                             const int* rS, int maxNnz, int rows, int baseIndex)
{
    switch (type) {
    case SPGPU_TYPE_FLOAT: return analyseForm<float, IS_HELL>(handle, rP, hackSize, hackOffsets, idxStride, rS, maxNnz, rows, baseIndex);
    case SPGPU_TYPE_DOUBLE: return analyseForm<double, IS_HELL>(handle, rP, hackSize, hackOffsets, idxStride, rS, maxNnz, rows, baseIndex);
    case SPGPU_TYPE_COMPLEX_FLOAT: return analyseForm<cfloat, IS_HELL>(handle, rP, hackSize, hackOffsets, idxStride, rS, maxNnz, rows, baseIndex);
    case SPGPU_TYPE_COMPLEX_DOUBLE: return analyseForm<cdouble, IS_HELL>(handle, rP, hackSize, hackOffsets, idxStride, rS, maxNnz, rows, baseIndex);
    default: return SPGPU_SPMV_FORM_AUTO;
    }
}

} // namespace spgpu

using namespace spgpu;

extern "C" {

/* Kept for callers that ask (the test suite's conftest): the lab build of non-default kernel shapes is retired, so always 0. */
int spgpuTuningVariantsBuilt(void)
{
    return 0;
}

int spgpuHellSpmvForm(spgpuHandle_t handle, spgpuType_t type, const int* rP, int hackSize, const int* hackOffsets, const int* rS, int rows,
                      int baseIndex)
{
    return analyseFormOfType<true>(handle, type, rP, hackSize, hackOffsets, hackSize, rS, 0, rows, baseIndex);
}

int spgpuHellSpmvPrepare(spgpuHandle_t handle, spgpuType_t type, const void* cM, const int* rP, int hackSize, const int* hackOffsets, const int* rS,
                         const int* rIdx, int rows, int baseIndex)
{
    if (!hackOffsets || !rS || hackSize <= 0)
        return SPGPU_UNSPECIFIED;
    return spgpu::prepareSpmvOfType<true>(handle, type, cM, rP, hackSize, hackOffsets, hackSize, hackSize, rS, rIdx, 0, rows, baseIndex);
}

int spgpuEllSpmvPrepare(spgpuHandle_t handle, spgpuType_t type, const void* cM, const int* rP, int cMPitch, int rPPitch, const int* rS, const int* rIdx,
                        int maxNnzPerRow, int rows, int baseIndex)
{
    return spgpu::prepareSpmvOfType<false>(handle, type, cM, rP, 0, nullptr, cMPitch, rPPitch, rS, rIdx, maxNnzPerRow, rows, baseIndex);
}

int spgpuHellSpmvFreeze(spgpuHandle_t handle, spgpuType_t type, const void* cM, const int* rP, int hackSize, const int* hackOffsets, const int* rS,
                        const int* rIdx, int rows, int baseIndex)
{
    if (!hackOffsets || !rS || hackSize <= 0)
        return SPGPU_UNSPECIFIED;
    return spgpu::prepareSpmvOfType<true>(handle, type, cM, rP, hackSize, hackOffsets, hackSize, hackSize, rS, rIdx, 0, rows, baseIndex, true);
}

int spgpuEllSpmvFreeze(spgpuHandle_t handle, spgpuType_t type, const void* cM, const int* rP, int cMPitch, int rPPitch, const int* rS, const int* rIdx,
                       int maxNnzPerRow, int rows, int baseIndex)
{
    return spgpu::prepareSpmvOfType<false>(handle, type, cM, rP, 0, nullptr, cMPitch, rPPitch, rS, rIdx, maxNnzPerRow, rows, baseIndex, true);
}

int spgpuEllSpmvForm(spgpuHandle_t handle, spgpuType_t type, const int* rP, int rPPitch, const int* rS, int maxNnzPerRow, int rows,
                     int baseIndex)
{
    return analyseFormOfType<false>(handle, type, rP, 0, nullptr, rPPitch, rS, maxNnzPerRow, rows, baseIndex);
}

#ifdef SPGPU_TRACE_BLOCKS
void spgpuPlannedSetTrace(unsigned long long* buffer);
void spgpuDebugSetTrace(unsigned long long* buffer)
{
    (void)hipMemcpyToSymbol(HIP_SYMBOL(spgpu::spgpuTraceBuffer), &buffer, sizeof(buffer));
    spgpuPlannedSetTrace(buffer);
}
#endif

void spgpuDebugCheck(spgpuHandle_t h, const char* what)
{
#ifdef SPGPU_DEBUG
    hipError_t err = hipStreamSynchronize(h->currentStream);
    if (err == hipSuccess)
        err = hipGetLastError();
    if (err != hipSuccess) {
        fprintf(stderr, "spgpu: HIP error in %s: %s\n", what, hipGetErrorString(err));
        exit(1);
    }
#else
    (void)h;
    (void)what;
#endif
}

/* avgNnzPerRow is a tuning hint in the reference (threads-per-row choice, hell_spmv_base_template.cuh:306-325); here it
 * selects the kernel without a prefetch ring when it says 1 .. 8 (launchSlabFamily); any value gives the same bits. */

void spgpuShellspmv(spgpuHandle_t handle, float* z, const float* y, float alpha, const float* cM,
                    const int* rP, int hackSize, const int* hackOffsets, const int* rS, const int* rIdx,
                    int avgNnzPerRow, int rows, const float* x, float beta, int baseIndex)
{
    hellSpmv<float>(handle, z, y, alpha, cM, rP, hackSize, hackOffsets, rS, rIdx, rows, x, beta, baseIndex, avgNnzPerRow);
}

void spgpuDhellspmv(spgpuHandle_t handle, double* z, const double* y, double alpha, const double* cM,
                    const int* rP, int hackSize, const int* hackOffsets, const int* rS, const int* rIdx,
                    int avgNnzPerRow, int rows, const double* x, double beta, int baseIndex)
{
    hellSpmv<double>(handle, z, y, alpha, cM, rP, hackSize, hackOffsets, rS, rIdx, rows, x, beta, baseIndex, avgNnzPerRow);
}

void spgpuChellspmv(spgpuHandle_t handle, hipFloatComplex* z, const hipFloatComplex* y, hipFloatComplex alpha,
                    const hipFloatComplex* cM, const int* rP, int hackSize, const int* hackOffsets,
                    const int* rS, const int* rIdx, int avgNnzPerRow, int rows, const hipFloatComplex* x,
                    hipFloatComplex beta, int baseIndex)
{
    hellSpmv<cfloat>(handle, z, y, alpha, cM, rP, hackSize, hackOffsets, rS, rIdx, rows, x, beta, baseIndex, avgNnzPerRow);
}

void spgpuZhellspmv(spgpuHandle_t handle, hipDoubleComplex* z, const hipDoubleComplex* y,
                    hipDoubleComplex alpha, const hipDoubleComplex* cM, const int* rP, int hackSize,
                    const int* hackOffsets, const int* rS, const int* rIdx, int avgNnzPerRow, int rows,
                    const hipDoubleComplex* x, hipDoubleComplex beta, int baseIndex)
{
    hellSpmv<cdouble>(handle, z, y, alpha, cM, rP, hackSize, hackOffsets, rS, rIdx, rows, x, beta, baseIndex, avgNnzPerRow);
}

void spgpuSellspmv(spgpuHandle_t handle, float* z, const float* y, float alpha, const float* cM, const int* rP,
                   int cMPitch, int rPPitch, const int* rS, const int* rIdx, int avgNnzPerRow,
                   int maxNnzPerRow, int rows, const float* x, float beta, int baseIndex)
{
    ellSpmv<float>(handle, z, y, alpha, cM, rP, cMPitch, rPPitch, rS, rIdx, maxNnzPerRow, rows, x, beta, baseIndex, avgNnzPerRow);
}

void spgpuDellspmv(spgpuHandle_t handle, double* z, const double* y, double alpha, const double* cM,
                   const int* rP, int cMPitch, int rPPitch, const int* rS, const int* rIdx, int avgNnzPerRow,
                   int maxNnzPerRow, int rows, const double* x, double beta, int baseIndex)
{
    ellSpmv<double>(handle, z, y, alpha, cM, rP, cMPitch, rPPitch, rS, rIdx, maxNnzPerRow, rows, x, beta, baseIndex, avgNnzPerRow);
}

void spgpuCellspmv(spgpuHandle_t handle, hipFloatComplex* z, const hipFloatComplex* y, hipFloatComplex alpha,
                   const hipFloatComplex* cM, const int* rP, int cMPitch, int rPPitch, const int* rS,
                   const int* rIdx, int avgNnzPerRow, int maxNnzPerRow, int rows, const hipFloatComplex* x,
                   hipFloatComplex beta, int baseIndex)
{
    ellSpmv<cfloat>(handle, z, y, alpha, cM, rP, cMPitch, rPPitch, rS, rIdx, maxNnzPerRow, rows, x, beta, baseIndex, avgNnzPerRow);
}

void spgpuZellspmv(spgpuHandle_t handle, hipDoubleComplex* z, const hipDoubleComplex* y, hipDoubleComplex alpha,
                   const hipDoubleComplex* cM, const int* rP, int cMPitch, int rPPitch, const int* rS,
                   const int* rIdx, int avgNnzPerRow, int maxNnzPerRow, int rows, const hipDoubleComplex* x,
                   hipDoubleComplex beta, int baseIndex)
{
    ellSpmv<cdouble>(handle, z, y, alpha, cM, rP, cMPitch, rPPitch, rS, rIdx, maxNnzPerRow, rows, x, beta, baseIndex, avgNnzPerRow);
}

/* alpha is accepted and not applied, as in the reference (ell_csput_base.cuh:35,44,66). */
void spgpuSellcsput(spgpuHandle_t handle, float alpha, float* cM, const int* rP, int cMPitch, int rPPitch, const int* rS,
                    int nnz, int* aI, int* aJ, float* aVal, int baseIndex)
{
    (void)alpha;
    ellCsput<float>(handle, cM, rP, cMPitch, rPPitch, rS, nnz, aI, aJ, aVal, baseIndex);
}
void spgpuDellcsput(spgpuHandle_t handle, double alpha, double* cM, const int* rP, int cMPitch, int rPPitch,
                    const int* rS, int nnz, int* aI, int* aJ, double* aVal, int baseIndex)
{
    (void)alpha;
    ellCsput<double>(handle, cM, rP, cMPitch, rPPitch, rS, nnz, aI, aJ, aVal, baseIndex);
}
void spgpuCellcsput(spgpuHandle_t handle, hipFloatComplex alpha, hipFloatComplex* cM, const int* rP, int cMPitch,
                    int rPPitch, const int* rS, int nnz, int* aI, int* aJ, hipFloatComplex* aVal, int baseIndex)
{
    (void)alpha;
    ellCsput<cfloat>(handle, cM, rP, cMPitch, rPPitch, rS, nnz, aI, aJ, aVal, baseIndex);
}
void spgpuZellcsput(spgpuHandle_t handle, hipDoubleComplex alpha, hipDoubleComplex* cM, const int* rP, int cMPitch,
                    int rPPitch, const int* rS, int nnz, int* aI, int* aJ, hipDoubleComplex* aVal, int baseIndex)
{
    (void)alpha;
    ellCsput<cdouble>(handle, cM, rP, cMPitch, rPPitch, rS, nnz, aI, aJ, aVal, baseIndex);
}

} // extern "C"
