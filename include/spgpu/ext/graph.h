#pragma once
/*
 * HOLDS: captured HIP graphs on planned, frozen and adopted matrices (no counterpart in the reference).
 *
 * A solver that multiplies by one matrix thousands of times has two answers in this library: a captured iteration
 * (spgpu/device_scalars.h; replayed with no host round trip) and the per-matrix records of spgpu/tuning.h -- plans
 * (spgpu?SpmvPrepare), frozen 16-bit index copies (spgpu?SpmvFreeze), adopted ordered copies (spgpu?SpmvAdopt).  A graph keeps
 * the device addresses its launches were captured with, and a record can be freed while the graph lives (spgpuSpmvThaw, the
 * least recently used of 8 records making room, a stale plan rebuilt): so, by default, launches captured into a graph use no
 * record and run as on a matrix the handle has never seen -- on an adopted ragged matrix the plain kernel on the caller's arrays
 * (2.7 ms against 0.71 on the north_star target).  A HOLD is the lifetime contract that lets them use it:
 *
 *     spgpuHellSpmvAdopt(h, ...);   (or Freeze / Prepare)
 *     spgpuSpmvHold(h, rP);
 *     ... capture the iteration (spgpu?hellspmv / spgpu?ellspmv on these arrays, on the handle's stream), replay it ...
 *     ... destroy the graphs (or never replay them again) ...
 *     spgpuSpmvRelease(h, rP);
 *     spgpuSpmvThaw(h, rP);
 *
 * spgpuSpmvHold takes a hold on every record the handle keeps under rP: the plans of the matrix, frozen or not, waited for if
 * still being built; the frozen record of a matrix without a row order; an adopted matrix' entry and the plan of its ordered
 * copy.  It synchronises the handle's current stream, like Prepare, Freeze and Adopt.
 *   SPGPU_SUCCESS      held;
 *   SPGPU_UNSUPPORTED  no usable record under rP (nothing prepared, frozen or adopted; SPGPU_PLAN=0; a plan given up) -- nothing
 *                      happens, captured calls run as before -- or the handle's current stream is capturing (the call then
 *                      neither waits nor disturbs the capture);
 *   SPGPU_UNSPECIFIED  a NULL argument.
 * Holds are counted: n Holds need n Releases.  spgpuSpmvRelease without a hold: SPGPU_UNSUPPORTED.  spgpuSpmvHolds: the current
 * count (0 if none).
 *
 * While a hold is on a matrix:
 *   - an ELL/HELL SpMV captured on the handle's stream whose arguments match a held record uses it, and runs exactly what the
 *     eager call runs (planned, packed or adopted kernels: the same bits).  spgpuSpmvPlanCounts' uses and spgpuSpmvAdoptedUses
 *     count such a launch once, at capture; replays do not count.  Records that are not held are not used in a capture;
 *   - the record is never evicted: a new matrix finds no room when all 8 records are held (its calls run without a plan, the
 *     same bits; Freeze, Prepare and Adopt of it say SPGPU_UNSUPPORTED), and never retired by the host;
 *   - spgpuSpmvThaw(h, rP) returns SPGPU_IN_USE and frees nothing (spgpuSpmvFrozenBytes unchanged); after the last Release it
 *     works as before.
 * The caller keeps Freeze's promise while the hold lasts -- rP, rS, hackOffsets and rIdx stay byte for byte as they are; for an
 * adopted matrix Adopt's: none of its arrays changes -- and releases only after the last graph that captured a launch on the
 * matrix has been destroyed or will not be replayed again.  Breaking the promise is undefined behaviour in the usual sense, as
 * for Freeze (spgpu/tuning.h).  spgpuDestroy frees every record, held or not: no graph captured from the handle may be replayed
 * after it.  Hold, Release and Holds are safe beside SpMV calls of other host threads on the handle.
 */
#include "../core.h"

#define SPGPU_IN_USE 4 /* spgpuSpmvThaw refused: a hold is on the matrix */

#ifdef __cplusplus
extern "C" {
#endif

int spgpuSpmvHold(spgpuHandle_t handle, const int* rP);
int spgpuSpmvRelease(spgpuHandle_t handle, const int* rP);
int spgpuSpmvHolds(spgpuHandle_t handle, const int* rP);

#ifdef __cplusplus
}
#endif
