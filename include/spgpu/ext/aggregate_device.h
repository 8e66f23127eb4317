#pragma once
/*
 * Aggregation for algebraic multigrid on CSR arrays, in HBM: strength of connection, the roots of the aggregates as a distance-2
 * maximal independent set (MIS-2) with fixed priorities, and the tentative prolongator T in CSR (the reference aggregates nothing,
 * and neither did this library).
 *
 * NEW: the producer of the prolongator that spgpu/ext/spgemm_device.h (the Galerkin product T^T * A * T) and spgpu/ext/add_device.h
 * (the smoothed P = T - w * (A * T)) were built to consume.  With it a second level is built from a matrix in HBM without an array
 * leaving the device (tools/amg_setup_amd.c).
 *
 * All array arguments are DEVICE pointers unless marked host.  Every call runs on handle->currentStream.
 *
 * THE CONTRACT
 * Matrix
 *   - one square CSR matrix of rowsCount rows with int indices and baseIndex 0 or 1;
 *   - columns need not ascend, a column may be stored twice, and a row may lack its diagonal;
 *   - d_i is |a_ii| of the first stored (i, i) of row i, and +0 if there is none.
 * Strength (spgpuCsrStrengthDevice)
 *   - real types only: valuesType is SPGPU_TYPE_FLOAT or SPGPU_TYPE_DOUBLE; anything else returns SPGPU_UNSUPPORTED before a launch;
 *   - writes diagAbs[i] = d_i, i < rowsCount, in the value type T;
 *   - writes strong[p], 0 or 1, for every stored entry p (row i, column j, value a_ij).  All arithmetic is in the value type and
 *     every operation is rounded separately (no fused multiply-add): t = (T)(theta*theta), the product formed in double on the host
 *     and converted once; lhs = a_ij*a_ij; rhs = (t*d_i)*d_j; strong[p] = (j != i) && lhs >= rhs;
 *   - a NaN on either side gives 0, because the comparison is false;
 *   - theta = 0 makes every finite stored off-diagonal entry between finite diagonals strong, a stored zero included;
 *   - a column outside [baseIndex, baseIndex + rowsCount) gives 0 and d_j is not read;
 *   - asynchronous, takes no scratch, keeps no state and can be captured into a HIP graph and replayed after the values changed in
 *     place; every byte has one writer, and a repeated call gives the same bytes.
 * Aggregation (spgpuCsrAggregateDevice)
 *   - S(i) is the set of the columns j != i of the entries p of row i with strong[p] != 0; with strong == NULL it is every stored
 *     j != i.  A node with empty S(i) is a root, and for a structurally symmetric S a singleton;
 *   - the priority of node i is hash(i) = lowbias32(i) >> 1, where lowbias32(x) is x ^= x>>16; x *= 0x7FEB352D; x ^= x>>15;
 *     x *= 0x846CA68B; x ^= x>>16 on 32-bit unsigned words;
 *   - the tuple of node i is (state, hash(i), i), ordered lexicographically, with OUT = 0 < UNDECIDED = 1 < ROOT = 2; it fits one
 *     64-bit word (2 + 31 + 31 bits).  All nodes start UNDECIDED;
 *   - a round is synchronous and goes from buffer to buffer: t0[i] is the tuple of i; t1[i] = max(t0[i], max over j in S(i) of
 *     t0[j]); t2[i] = max(t1[i], max over j in S(i) of t1[j]).  An undecided i with t2[i] == t0[i] becomes ROOT; otherwise, if the
 *     state of t2[i] is ROOT, it becomes OUT; otherwise it stays UNDECIDED;
 *   - rounds repeat until no node is undecided.  The undecided node with the largest tuple always decides (whatever exceeds its
 *     tuple is a ROOT), so the process ends; *roundsCount receives the number of rounds;
 *   - roots are numbered 0-based by ascending row with one exclusive scan; *aggregatesCount is their number;
 *   - two joining passes follow, each reading only the previous pass's array.  Pass 1: a non-root with an assigned node in S(i)
 *     takes the smallest such aggregate number.  Pass 2: the same for the nodes still unassigned, reading pass 1's result;
 *   - every node is assigned after pass 2: a non-root i went OUT in a round in which t2[i] was a ROOT's tuple, so a root r lies at
 *     the end of a path i -> j -> r with j in S(i) or j = i, and r in S(j) or r = j.  Pass 1 assigns j (it is a root, or it has the
 *     root r in S(j)), and pass 2 assigns i (it has the assigned j in S(i), or it is j);
 *   - aggregateOf[i], i < rowsCount, is 0-based whatever baseIndex is; aggregateSize[a] is the number of nodes of aggregate a and
 *     is written for a < *aggregatesCount: nothing beyond it is touched;
 *   - for a structurally symmetric S the roots are the unique MIS-2 that a greedy pass in descending tuple order gives: no two
 *     roots lie within distance 2 and every node has a root within distance 2.  For an unsymmetric S the rounds are the
 *     definition;
 *   - max and min are exact, so no result depends on scheduling, on the kernel shape or on the grid, a repeated call gives the
 *     same bytes, and numpy can restate them (spgpu_amd.formats.csr_aggregate): the tests compare bytes.  The only atomic is the
 *     integer count of the nodes still undecided; no floating-point atomics are used;
 *   - the call synchronises the stream about once per round (it returns host data) and cannot be captured;
 *   - `work` is caller-provided scratch of spgpuCsrAggregateWorkBytes(rowsCount) bytes, 256-byte aligned -- about 32 bytes per
 *     row, with no share of the entries.  It may be freed once the call has returned.
 * Refusals: SPGPU_UNSUPPORTED from the aggregation with *aggregatesCount = 0 and *roundsCount = 0, reported after the synchronise
 * with nothing read or written out of bounds; aggregateOf and aggregateSize then have no defined content
 *   - a strong entry, or any entry when strong == NULL, with a column outside [baseIndex, baseIndex + rowsCount).  The offending
 *     entry is clamped out (it is no neighbour) and a flag is raised, as the Plan of spgpu/ext/trsv_device.h does.
 * Tentative prolongator (spgpuCsrTentativeDevice)
 *   - tRowPtr[i] = i + baseIndex for i <= rowsCount; tColIndices[i] = aggregateOf[i] + baseIndex; tValues[i] is the bits of
 *     candidate[i], -0.0 and NaN payloads included, or 1 of the type when candidate == NULL;
 *   - valuesType is SPGPU_TYPE_FLOAT, _DOUBLE, _COMPLEX_FLOAT or _COMPLEX_DOUBLE; anything else returns SPGPU_UNSUPPORTED before a
 *     launch;
 *   - asynchronous, takes no scratch, keeps no state and can be captured;
 *   - T has rowsCount rows, *aggregatesCount columns and one ascending column per row: it is directly an operand of
 *     spgpuCsrSpgemm* and spgpuCsrAdd*.
 * Degenerate inputs
 *   - rowsCount <= 0: every call returns SPGPU_SUCCESS with nothing launched; the aggregation sets both counts to 0;
 *   - a null output, a null matrix array where it is read, or a null `work` with rows to do: SPGPU_UNSUPPORTED before a launch (the
 *     aggregation sets both counts to 0).
 * State
 *   - no call allocates or keeps state; no kernel waits for another workgroup: rounds, sweeps and passes are ordered by stream order
 *     between launches, nothing else.
 *
 * A second level from a matrix in HBM (A in CSR, fp64):
 *
 *     spgpuCsrStrengthDevice(h, strong, diagAbs, rows, aPtr, aIdx, aVal, base, 0.25, SPGPU_TYPE_DOUBLE);
 *     spgpuCsrAggregateDevice(h, &aggregates, &rounds, aggregateOf, aggregateSize, rows, aPtr, aIdx, strong, base, work);
 *     spgpuCsrTentativeDevice(h, tPtr, tIdx, tVal, rows, aggregateOf, NULL, base, SPGPU_TYPE_DOUBLE);
 *     (T^T through spgpuCsrToHellDevice, spgpuHellTransposeDevice and spgpuHellToCsrDevice; A_c = (T^T * A) * T through
 *      spgpu/ext/spgemm_device.h)
 */
#include "../core.h"

#ifdef __cplusplus
extern "C" {
#endif

/* NEW (no counterpart in the reference).  Bytes of scratch for spgpuCsrAggregateDevice; monotone in rowsCount, and the same for
 * rowsCount <= 0 as for rowsCount == 0. */
size_t spgpuCsrAggregateWorkBytes(int rowsCount);

/* NEW (no counterpart in the reference).  strong[p] for every stored entry and diagAbs[i] for every row.  Asynchronous, no
 * scratch, no state. */
spgpuStatus_t spgpuCsrStrengthDevice(spgpuHandle_t handle, __device unsigned char* strong, __device void* diagAbs, int rowsCount,
                                     const __device int* rowPtr, const __device int* colIndices, const __device void* values,
                                     int baseIndex, double theta, spgpuType_t valuesType);

/* NEW (no counterpart in the reference).  The aggregates of the graph S.  Synchronises the stream about once per round (returns
 * host data).  Writes aggregateOf[rowsCount] and the first *aggregatesCount ints of aggregateSize (rowsCount ints hold every
 * case).  strong == NULL: every stored off-diagonal entry. */
spgpuStatus_t spgpuCsrAggregateDevice(spgpuHandle_t handle, __host int* aggregatesCount, __host int* roundsCount,
                                      __device int* aggregateOf, __device int* aggregateSize, int rowsCount, const __device int* rowPtr,
                                      const __device int* colIndices, const __device unsigned char* strong, int baseIndex,
                                      __device void* work);

/* NEW (no counterpart in the reference).  T in CSR: tRowPtr[rowsCount + 1], tColIndices[rowsCount], tValues[rowsCount].
 * candidate == NULL: ones.  Asynchronous, no scratch, no state. */
spgpuStatus_t spgpuCsrTentativeDevice(spgpuHandle_t handle, __device int* tRowPtr, __device int* tColIndices, __device void* tValues,
                                      int rowsCount, const __device int* aggregateOf, const __device void* candidate, int baseIndex,
                                      spgpuType_t valuesType);

#ifdef __cplusplus
}
#endif
